/*
 * librecnow_hip.so -- C ABI of the MI355X (gfx950) implementation of rec_now's in-batch ranking-loss and
 * feature-interaction hot path.
 *
 * The reference (ChaoLiangTHU/rec_now) is pure Python on TensorFlow: it has NO FFI/plugin layer, so there is no
 * reference C interface to copy.  Each entry point below therefore cites the reference PYTHON function/lines whose
 * arithmetic it replaces; the Python mirror of the reference's own call signatures lives in rec_now_amd/ and reaches
 * these symbols through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is DEVICE memory (hipMalloc'ed / torch CUDA tensor storage) unless
 *     the parameter name ends in _host.  The caller owns every buffer; the library never allocates or frees.
 *   - every entry point is asynchronous on `stream` (a hipStream_t passed as void*), stateless and re-entrant -- with the three
 *     process-wide settings and the one host-side note listed under "Library state" below.
 *   - return value: 0 = ok, negative = RECNOW_E*, positive = a forwarded hipError_t.  No C++ exception crosses.
 *   - scratch memory: `*_workspace_bytes(...)` is queried first, the caller passes `ws`/`ws_bytes`.
 *   - all matrices are row-major, fp32 unless stated; index outputs are int32, counts are int64.
 *   - reductions are deterministic (no floating-point atomics anywhere): same inputs -> same bits.
 */
#ifndef RECNOW_H_
#define RECNOW_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RECNOW_OK 0
#define RECNOW_EINVAL (-1)       /* bad argument (null pointer, negative size, unsupported combination) */
#define RECNOW_EWORKSPACE (-2)   /* ws_bytes smaller than *_workspace_bytes() */
#define RECNOW_EUNSUPPORTED (-3) /* shape outside what the kernels implement (documented per function) */

/* activations fused into kernels (keras names: None/'linear', 'relu', 'tanh', 'sigmoid') */
#define RECNOW_ACT_LINEAR 0
#define RECNOW_ACT_RELU 1
#define RECNOW_ACT_TANH 2
#define RECNOW_ACT_SIGMOID 3

/* group-id dtypes accepted by recnow_group_keys */
#define RECNOW_KEY_F32 0
#define RECNOW_KEY_F64 1
#define RECNOW_KEY_I32 2
#define RECNOW_KEY_I64 3
/* OR-ed into one of the four above: float ids compare as tf.unique does (listwise_loss_from_batch.py:109) -- equal infinities are
 * one group, only NaN rows are solo.  Without it they follow `g_i - g_j == 0.0` of the pairwise loss: +-inf pair with nobody. */
#define RECNOW_KEY_INF_EQUAL 256

/* pair predicate flags */
#define RECNOW_PAIR_LABEL_GT 1    /* keep (i,j) only if label_i > label_j   (pairwise_loss_from_batch.py:189)     */
#define RECNOW_PAIR_WRONG_ORDER 2 /* keep (i,j) only if score_i < score_j   (pairwise_loss_from_batch.py:197-203) */
#define RECNOW_PAIR_MEMBERS_PACKED 256 /* recnow_pair_bpr_fwdbwd (and recnow_pair_count after recnow_group_pack_small): the workspace is the one recnow_pair_count just
                                          used with the same scores / labels / mask / order -- its packed rows are reused */

int recnow_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * Grouping: replaces the dense (B,B) same-group mask of rec_now/rec_block/pairwise_loss_from_batch.py:16-40,43-74
 * and tf.unique_with_counts of listwise_loss_from_batch.py:109 by canonical keys + stable radix sort + segments.
 * ---------------------------------------------------------------------------------------------------------- */

/* Number of 32-bit key words one group tensor of `dtype` (with or without RECNOW_KEY_INF_EQUAL) contributes (1 or 2); <0 on bad dtype. */
int recnow_key_words(int dtype);

/* Canonicalise one group-id tensor into key words.  Float semantics follow `g_i - g_j == 0.0`
 * (pairwise_loss_from_batch.py:33-35): -0.0 == +0.0; NaN and +-inf rows pair with nobody -> solo[i] |= 1.
 * dtype | RECNOW_KEY_INF_EQUAL: tf.unique equality instead -- only NaN rows are solo, all +inf rows are one group, all -inf rows another.
 * words: [recnow_key_words(dtype)][B] (word-major, most significant word first).  solo: [B], OR-accumulated. */
int recnow_group_keys(const void* group, int dtype, int64_t B, uint32_t* words, uint8_t* solo, void* stream);

size_t recnow_group_segments_workspace_bytes(int64_t B, int n_words);

/* Stable LSD radix sort of rows by the composite key (all words, lexicographic) and segment detection.
 *   words        [n_words][B]  composite key, words of groups[0] first (n_words_first of them)
 *   solo         [B]           rows that pair with nobody (each becomes a segment of its own)
 * outputs
 *   order        [B]    original row index at sorted position k (ascending row index inside a segment)
 *   seg_id       [B]    segment (= group) index of sorted position k, segments numbered in sorted order
 *   seg_first    [B+1]  first sorted position of segment g; seg_first[n_seg] = B
 *   super_id     [B]    index of the groups[0]-only segment containing sorted position k
 *   n_seg        [2]    {number of segments, number of groups[0]-only segments}
 */
int recnow_group_segments(const uint32_t* words, const uint8_t* solo, int64_t B, int n_words, int n_words_first,
                          int32_t* order, int32_t* seg_id, int32_t* seg_first, int32_t* super_id, int32_t* n_seg,
                          void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * In-batch pairwise loss: rec_now/rec_block/pairwise_loss_from_batch.py
 * ---------------------------------------------------------------------------------------------------------- */
size_t recnow_pairwise_workspace_bytes(int64_t B);

/* Per-row count of valid partners (replaces the mask algebra of pairwise_loss_from_batch.py:254-264).
 *   valid(i,j) = same segment, i != j, mask_i && mask_j, [label_i > label_j], [score_i < score_j]
 *   cnt_row   [B]  c_i by ORIGINAL row index
 *   cnt_super [B]  number of surviving pairs whose positive row lies in groups[0]-segment s  (:282-291)
 *   n_pair    [1]
 * mask may be NULL (all rows valid). */
int recnow_pair_count(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order,
                      const int32_t* seg_id, const int32_t* seg_first, const int32_t* super_id, int64_t B, int flags,
                      int32_t* cnt_row, int64_t* cnt_super, int64_t* n_pair, void* ws, size_t ws_bytes, void* stream);

/* Exclusive scan of cnt_row over ORIGINAL row order -> offsets[B+1] (offsets[B] = n_pair). */
int recnow_pair_offsets(const int32_t* cnt_row, int64_t B, int64_t* offsets, void* ws, size_t ws_bytes, void* stream);

/* Materialise the pair list in the reference's order: row-major over the dense mask = ascending i, then ascending j
 * (tf.boolean_mask of the flattened (B,B) mask, pairwise_loss_from_batch.py:217,272-273).  Bit-exact integer path.
 * pos_idx/neg_idx: [capacity]; pairs beyond capacity are not written. */
int recnow_pair_emit(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order,
                     const int32_t* seg_id, const int32_t* seg_first, int64_t B, int flags, const int64_t* offsets,
                     int32_t* pos_idx, int32_t* neg_idx, int64_t capacity, void* ws, size_t ws_bytes, void* stream);

/* Fused BPR/logistic pairwise loss + gradient without materialising pairs (pairwise_loss_from_batch.py:96-127 applied
 * to the pair set of :254-274; occurrence weights of :130-151,282-291).
 *   loss   = sum_p w_p * softplus(-factor*(s_i - s_j)) / (float(P) + 1e-10)      (or the raw sum if !reduce_mean)
 *   w_p    = cnt_super[super(i_p)] ** power   (power == 0 -> 1)
 *   dscores[k] = d loss / d scores[k]   (pair set and weights are constants, :264,:270)
 * loss: [1] fp32, dscores: [B].
 * flags must contain RECNOW_PAIR_LABEL_GT or RECNOW_PAIR_WRONG_ORDER (else RECNOW_EINVAL): the fused walk relies on at most
 * one of (i,j) / (j,i) being a pair.  Pair sets without either predicate go through recnow_pair_emit + recnow_bpr_loss_fwdbwd. */
int recnow_pair_bpr_fwdbwd(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order,
                           const int32_t* seg_id, const int32_t* seg_first, const int32_t* super_id,
                           const int64_t* cnt_super, const int64_t* n_pair, int64_t B, int flags, float factor,
                           float power, int reduce_mean, float* loss, float* dscores, void* ws, size_t ws_bytes,
                           void* stream);

/* The same loss WITHOUT occurrence weights (click_occurance_power == 0, the reference's default) in one walk per row: pair counts and
 * BPR terms come out of the same pass (no recnow_pair_count before it).  n_pair (out, [1]) = P; loss = sum / (P + 1e-10) or the raw
 * sum; dscores_unnorm[k] = d(SUM of pair losses) / d scores[k], i.e. NOT divided by P: multiply the incoming gradient in with
 * recnow_pair_scale_grad, which applies 1 / (P + eps) as well (n_pair = NULL there for the raw sum).  flags as recnow_pair_bpr_fwdbwd
 * (RECNOW_PAIR_MEMBERS_PACKED after recnow_group_pack_small on the same ws). */
int recnow_pair_bpr_onepass(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order,
                            const int32_t* seg_id, const int32_t* seg_first, int64_t B, int flags, float factor, int reduce_mean,
                            float* loss, float* dscores_unnorm, int64_t* n_pair, void* ws, size_t ws_bytes, void* stream);
/* out[i] = dscores_unnorm[i] * g[0] / (float(*n_pair) + eps); g a DEVICE scalar (the gradient of the loss); n_pair == NULL: no division. */
int recnow_pair_scale_grad(const float* dscores_unnorm, const float* g, const int64_t* n_pair, float eps, int64_t B, float* out,
                           void* stream);

/* The pair set and weights of a label_pair_to_weight_func (pairwise_loss_from_batch.py:175-194) over labels that take at most 16 distinct
 * values, as a table: label_values [n_values] (distinct, finite), table [n_values x n_values] row-major, both DEVICE pointers;
 * table[a][b] is the weight of a pair whose positive row has label label_values[a] and whose negative row has label_values[b].  (i, j) is a
 * pair where the weight is > 0 (:193; zero, negative and NaN drop it, +inf keeps it), AND-ed per direction with score_i < score_j under
 * RECNOW_PAIR_WRONG_ORDER -- the only predicate flag these take.  Both (i, j) and (j, i) may be pairs.  n_values outside 1..16:
 * RECNOW_EINVAL.  A row that takes part (mask) with a label outside label_values makes the loss and every dscores entry NaN.
 *   recnow_pair_table_count        outputs as recnow_pair_count (cnt_row / cnt_super by the positive row); leaves the members (with their class
 *                                  ids) packed in ws
 *   recnow_pair_table_bpr_fwdbwd   outputs as recnow_pair_bpr_fwdbwd, each pair weighted table[a][b] * cnt_super[super(i)] ** power; n_pair /
 *                                  cnt_super from recnow_pair_table_count on the same inputs; RECNOW_PAIR_MEMBERS_PACKED: on the same ws, too. */
int recnow_pair_table_count(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order,
                            const int32_t* seg_id, const int32_t* seg_first, const int32_t* super_id, int64_t B, int flags,
                            const float* label_values, int n_values, const float* table, int32_t* cnt_row, int64_t* cnt_super,
                            int64_t* n_pair, void* ws, size_t ws_bytes, void* stream);
int recnow_pair_table_bpr_fwdbwd(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order,
                                 const int32_t* seg_id, const int32_t* seg_first, const int32_t* super_id,
                                 const int64_t* cnt_super, const int64_t* n_pair, int64_t B, int flags,
                                 const float* label_values, int n_values, const float* table, float factor, float power,
                                 int reduce_mean, float* loss, float* dscores, void* ws, size_t ws_bytes, void* stream);

/* The fused pairwise loss for pair terms other than BPR: the `pairloss_func` of pairwise_loss (pairwise_loss_from_batch.py:228-279) as one of
 *   RECNOW_PAIR_KIND_HINGE            f(u) = max(u, 0)        (subgradient 0 at u == 0)
 *   RECNOW_PAIR_KIND_SQUARED_HINGE    f(u) = max(u, 0) ** 2
 *   RECNOW_PAIR_KIND_MARGIN_LOGISTIC  f(u) = softplus(u)
 * of u = margin - factor * (s_i - s_j) per pair (i, j):
 *   loss = sum_p w_p f(u_p) / (float(P) + 1e-10)   (or the raw sum if !reduce_mean),   dscores[k] = d loss / d scores[k]
 * The pair set and w_p follow `table`:
 *   table != NULL  label_values / n_values / table as recnow_pair_table_count; w_p = table[a][b] * cnt_super[super(i_p)] ** power; flags:
 *                  [RECNOW_PAIR_WRONG_ORDER]; n_pair / cnt_super from recnow_pair_table_count on the same inputs.  A row that takes part with a
 *                  label outside label_values makes the loss and every dscores entry NaN.
 *   table == NULL  the rule label_i > label_j: flags must hold RECNOW_PAIR_LABEL_GT [| RECNOW_PAIR_WRONG_ORDER]; w_p = cnt_super[super(i_p)] **
 *                  power; n_pair / cnt_super from recnow_pair_count with the same flags; label_values / n_values are not looked at.
 * RECNOW_PAIR_MEMBERS_PACKED: ws is the workspace that count call just used (its packed rows are reused); without it the rows are packed here.
 * Workspace: recnow_pairwise_workspace_bytes(B).  RECNOW_EINVAL: an unknown kind, a non-finite margin or factor, n_values outside 1..16 with a
 * table, table == NULL without RECNOW_PAIR_LABEL_GT, any other flag, power != 0 without cnt_super.  B == 0 writes loss = 0. */
#define RECNOW_PAIR_KIND_HINGE 1
#define RECNOW_PAIR_KIND_SQUARED_HINGE 2
#define RECNOW_PAIR_KIND_MARGIN_LOGISTIC 3
int recnow_pair_kind_fwdbwd(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order,
                            const int32_t* seg_id, const int32_t* seg_first, const int32_t* super_id, const int64_t* cnt_super,
                            const int64_t* n_pair, int64_t B, int flags, int kind, float margin, const float* label_values, int n_values,
                            const float* table, float factor, float power, int reduce_mean, float* loss, float* dscores, void* ws,
                            size_t ws_bytes, void* stream);

/* The NDCG (LambdaRank) pair weight of the fused pairwise loss, and the in-batch NDCG.  A list is one segment; only rows that take part (mask)
 * are ranked.  Position of row i, from 0:  r_i = #{ j in the list, taking part, j != i : s_j > s_i or (s_j == s_i and j < i) }  (original row
 * indices break ties, so the positions form a permutation); q_i: the same count on the labels.
 *   D(r) = 1 / log2(2 + r), and 0 for r >= topn when topn > 0;   G(y) = 2**y - 1 (RECNOW_NDCG_GAIN_EXP2) or y (RECNOW_NDCG_GAIN_LINEAR)
 *   DCG = sum G(y_i) D(r_i),  IDCG = sum G(y_i) D(q_i) per list (fp64, fixed order),  inv = 1 / IDCG where IDCG > 0, else 0
 *   lambda_ij = |G(y_i) - G(y_j)| * |D(r_i) - D(r_j)| * inv(list)
 * recnow_pair_lambda_terms  ranks every row (one compare-only traversal of each segment) and leaves {D(r_i), G(y_i)} and inv per sorted row in
 *   `ws`.  Outputs, each optional (NULL): rank [B] int32 (-1: the row does not take part), discount / gain / inv_idcg [B] float32, all by
 *   ORIGINAL row; list_dcg / list_idcg [B] fp64 by segment (the first n_seg entries are written); ndcg_mean [1] = mean of DCG / IDCG over the
 *   lists with IDCG > 0 (0 when there is none), n_lists [1] = their number.  flags: 0 -- the rows are packed here from scores / labels / mask /
 *   order --, or RECNOW_PAIR_MEMBERS_PACKED: ws is the workspace recnow_pair_count / recnow_pair_table_count just used on these inputs (scores,
 *   labels, mask and order are then not looked at).  topn <= 0: no cut-off.  No host synchronisation; bitwise reproducible.
 * recnow_pair_lambda_fwdbwd  the loss of recnow_pair_kind_fwdbwd (same kinds, pair rules, flags, n_pair / cnt_super and NaN rule; BPR is
 *   RECNOW_PAIR_KIND_MARGIN_LOGISTIC at margin 0) with every pair's weight multiplied by lambda_ij.  The pair set is untouched: a pair with
 *   lambda == 0 still counts in n_pair.  flags MUST hold RECNOW_PAIR_MEMBERS_PACKED: ws is the workspace on which the matching count call and then
 *   recnow_pair_lambda_terms (with RECNOW_PAIR_MEMBERS_PACKED) have just run.
 * Workspace of both, and of the count call in front of them: recnow_pair_lambda_workspace_bytes(B) (it begins with the pairwise workspace). */
#define RECNOW_NDCG_GAIN_EXP2 0
#define RECNOW_NDCG_GAIN_LINEAR 1
size_t recnow_pair_lambda_workspace_bytes(int64_t B);
int recnow_pair_lambda_terms(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order, const int32_t* seg_id,
                             const int32_t* seg_first, int64_t B, int flags, int gain, int topn, int32_t* rank, float* discount,
                             float* gain_out, float* inv_idcg, double* list_dcg, double* list_idcg, float* ndcg_mean, int64_t* n_lists,
                             void* ws, size_t ws_bytes, void* stream);
int recnow_pair_lambda_fwdbwd(const int32_t* seg_id, const int32_t* seg_first, const int32_t* super_id, const int64_t* cnt_super,
                              const int64_t* n_pair, int64_t B, int flags, int kind, float margin, int n_values, const float* table,
                              float factor, float power, int reduce_mean, float* loss, float* dscores, void* ws, size_t ws_bytes,
                              void* stream);

/* In-batch GAUC: the AUC of every list, averaged over the lists, from exact integer pair counts (one compare-only traversal of each segment).
 * Lists and rows.  A list is one segment of build_segments(groups).  Only rows that take part are looked at.  A row takes part when mask is
 *   true, or when no mask is given.
 * Pairs.  For two distinct taking-part rows i, j of one list, (i, j) is a pair
 *   - under the graded rule (binary == 0), when label_i > label_j: the concordance index for graded labels; for 0/1 labels the AUC;
 *   - under the binary rule (binary != 0), when label_i > th and not (label_j > th), th = pos_neg_th, a finite float.
 *   Comparisons are float32 and IEEE: a NaN label is in no pair under the graded rule and is a negative under the binary rule.
 * Per-row counts, kept by row i as the higher side of the pair, int32:  n_i = number of j for which (i, j) is a pair, c_i = number of pairs
 *   with s_i > s_j, t_i = number of pairs with s_i == s_j.  A NaN score makes both comparisons false, so that pair counts as discordant.  A
 *   row that does not take part holds 0, 0, 0.
 * Per-list counts.  N, C, T are the int64 sums of n_i, c_i, t_i over the list, R is the number of taking-part rows.  The list's AUC is
 *   (2C + T) / (2N), formed in fp64 from the integers, for lists with N > 0.  Lists with N = 0 have no AUC and are left out of every batch mean.
 * Batch metric.  sum_L w_L AUC_L / sum_L w_L over the lists with N > 0;  w_L = R (RECNOW_AUC_WEIGHT_ROWS: impressions-weighted GAUC), N
 *   (RECNOW_AUC_WEIGHT_PAIRS: the pooled share of correctly ordered pairs) or 1 (RECNOW_AUC_WEIGHT_UNIFORM).  0 when no list has N > 0.  The
 *   sums are fp64 in a fixed order.
 * Outputs, each optional (NULL): row_n / row_c / row_t [B] int32 by ORIGINAL row; list_n / list_c / list_t / list_rows [B] int64 by segment
 *   (the first n_seg entries are written); auc [1] float32; weighted_sum / weight_sum [1] fp64 (numerator and denominator of auc);
 *   n_lists [1] int64 = the number of lists with N > 0.
 * flags: 0 -- the rows are packed here from scores / labels / mask / order --, or RECNOW_PAIR_MEMBERS_PACKED: ws is the workspace
 *   recnow_pair_count / recnow_pair_table_count just used on these inputs (scores, labels, mask and order are then not looked at).
 * Workspace: recnow_pair_auc_workspace_bytes(B) (it begins with the pairwise workspace).  RECNOW_EINVAL: an unknown weight kind, any other flag,
 *   a non-finite pos_neg_th with binary, NULL segment arrays with B > 0; RECNOW_EWORKSPACE: a workspace that is too small.  B == 0 writes
 *   auc = 0, zero sums and n_lists = 0.  No host synchronisation; bitwise reproducible. */
#define RECNOW_AUC_WEIGHT_ROWS 0
#define RECNOW_AUC_WEIGHT_PAIRS 1
#define RECNOW_AUC_WEIGHT_UNIFORM 2
size_t recnow_pair_auc_workspace_bytes(int64_t B);
int recnow_pair_auc_terms(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order, const int32_t* seg_id,
                          const int32_t* seg_first, int64_t B, int flags, int binary, float pos_neg_th, int weight_kind, int32_t* row_n,
                          int32_t* row_c, int32_t* row_t, int64_t* list_n, int64_t* list_c, int64_t* list_t, int64_t* list_rows, float* auc,
                          double* weighted_sum, double* weight_sum, int64_t* n_lists, void* ws, size_t ws_bytes, void* stream);

/* The same counts and metric WITHOUT a walk over the pairs (ABI 22): every list is sorted by score (recnow_group_segments on the key words
 * {seg_id, order-preserving image of the score}, called inside on this entry's workspace) and the counts of a row are differences of per-class
 * prefix counts at the ends of its list and of its run of tied scores.  O(B log B) whatever the list lengths; the walk is quadratic in them.
 * Arguments, definitions, outputs, return codes and the B == 0 case are those of recnow_pair_auc_terms, and for every input it accepts the
 * integers are the same, so the fp64 sums and the metric are bit-identical too.  Differences:
 *   - flags must be 0: RECNOW_PAIR_MEMBERS_PACKED is refused (RECNOW_EINVAL) -- this route reads no member records.
 *   - classes.  Binary rule: two classes, any labels.  Graded rule: the classes are the distinct non-NaN label values of the taking-part rows of
 *     the batch (-0.0 == +0.0), found on the device; up to 16 are supported.
 *   - poisoning.  With more than 16 values, or when the inner grouping call reports a grid-barrier time-out (its n_seg[0] < 0), the host cannot
 *     be told without a synchronisation, so every output asked for is overwritten: auc, weighted_sum, weight_sum = NaN, n_lists = -1, and all B
 *     entries of every per-row and per-list count = -1.
 * Workspace: recnow_pair_auc_sorted_workspace_bytes(B) (its own layout: it does NOT begin with the pairwise workspace; at most 16 int32 per row
 *   beside the sort's).  No host synchronisation; integer counting only; bitwise reproducible; every launch can be captured in a HIP graph.
 * RECNOW_AUC_SORT_TILE: positions of the (list, score) order per workgroup of the prefix-count kernels (tests restate their census from it). */
#define RECNOW_AUC_SORT_TILE 1024
size_t recnow_pair_auc_sorted_workspace_bytes(int64_t B);
int recnow_pair_auc_sorted_terms(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order, const int32_t* seg_id,
                                 const int32_t* seg_first, int64_t B, int flags, int binary, float pos_neg_th, int weight_kind, int32_t* row_n,
                                 int32_t* row_c, int32_t* row_t, int64_t* list_n, int64_t* list_c, int64_t* list_t, int64_t* list_rows,
                                 float* auc, double* weighted_sum, double* weight_sum, int64_t* n_lists, void* ws, size_t ws_bytes,
                                 void* stream);

/* pairwise_loss(outputs, labels, groups) with the reference's defaults (pairloss_func = bpr_loss_func, click_occurance_power = 0,
 * one group tensor; rec_block/pairwise_loss_from_batch.py:228-279) as ONE call: grouping (the single-launch front end when
 * recnow_pairwise_small_supported, else keys + radix sort + segments), the one-walk loss and the gradient
 *   dscores[k] = d loss / d scores[k]   (already divided by P + 1e-10 when reduce_mean),
 * so that a host framework's backward is one multiply by the incoming gradient.  One workspace holds every intermediate
 * (recnow_pairwise_loss_workspace_bytes); out2 (2 floats, optional) receives {loss, (float) P} beside loss / n_pair.
 * flags: RECNOW_PAIR_LABEL_GT [| RECNOW_PAIR_WRONG_ORDER].  mask may be NULL. */
size_t recnow_pairwise_loss_workspace_bytes(int64_t B, int key_dtype);
int recnow_pairwise_loss(const void* groups, int key_dtype, const float* labels, const float* scores, const uint8_t* mask, int64_t B,
                         int flags, float factor, int reduce_mean, float* loss, int64_t* n_pair, float* out2, float* dscores, void* ws,
                         size_t ws_bytes, void* stream);

/* Front end of the loss for a SMALL batch in one launch (BASELINE config 2: pairwise_loss_from_batch at B = 8192): canonical keys
 * of ONE float32 / int32 group tensor (key_dtype RECNOW_KEY_F32 / RECNOW_KEY_I32), stable sort and segments by a single
 * 1024-thread workgroup on LDS-resident keys, B <= 8192 (recnow_pairwise_small_supported), plus what recnow_pair_count would do
 * first: the packed member records in `ws` (recnow_pairwise_workspace_bytes) and cleared cnt_super[0..B) / *n_pair.  Follow with
 * recnow_pair_count and recnow_pair_bpr_fwdbwd on the SAME ws with RECNOW_PAIR_MEMBERS_PACKED in flags.  Same outputs as
 * recnow_group_keys + recnow_group_segments on these ids. */
int recnow_pairwise_small_supported(int64_t B, int key_dtype);
int recnow_group_pack_small(const void* groups, int key_dtype, const float* labels, const float* scores, const uint8_t* mask,
                            int64_t B, int32_t* order, int32_t* seg_id, int32_t* seg_first, int32_t* super_id, int32_t* n_seg,
                            int64_t* cnt_super, int64_t* n_pair, void* ws, size_t ws_bytes, void* stream);

/* bpr_loss_func on explicit (P,) vectors (pairwise_loss_from_batch.py:96-127).  weights may be NULL.
 * dpos = d loss/d outputs_pos, dneg = -dpos.  P may be 0 (loss = 0). */
int recnow_bpr_loss_fwdbwd(const float* pos, const float* neg, const float* weights, int64_t P, float factor,
                           int reduce_mean, float* loss, float* dpos, void* ws, size_t ws_bytes, void* stream);

/* Dense (B,B) bool mask, for API parity with generate_pair_mask (pairwise_loss_from_batch.py:43-74).
 * only_upper_band keeps only j == i+1 (band_part(m,0,1) minus the diagonal, :38-39).  mask_out must be zero-filled. */
int recnow_pair_mask_dense(const int32_t* order, const int32_t* seg_id, const int32_t* seg_first, int64_t B,
                           int only_upper_band, uint8_t* mask_out, void* stream);

/* occurance_power_weight (pairwise_loss_from_batch.py:130-151): w[i] = (size of i's segment) ** power. */
int recnow_occurance_power_weight(const int32_t* order, const int32_t* seg_id, const int32_t* seg_first, int64_t B,
                                  float power, float* w_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * In-batch listwise loss: rec_now/rec_block/listwise_loss_from_batch.py:89-173 on sorted segments (no (G,B) matrix).
 *   lists: the rows tf.unique (:109) finds equal -- -0.0 == +0.0, equal infinities equal, every NaN alone (RECNOW_KEY_INF_EQUAL)
 *   valid group g: has a label > th and a (label - th) < 0 (:135-137), both over the PADDED row of the reference's (G,B) matrix:
 *       with th < 0 the zero labels of the padding make every list shorter than the batch one with a positive;  p_i = y_i / sum_g y (:144)
 *   row g of the reference's dense logits = members' logits + (B - n_g) entries equal to pad_logit
 *       (pad_logit = value_of_masked_logit when do_mask_logits, else 0; :139-140)
 *   l_g = lse(row g) * sum_i p_i - sum_i p_i s_i (:167);  loss = mean over valid groups of w_g l_g, NaN -> 0 (:168-172)
 * Segment arrays are sized B and indexed by segment; valid_rank[g] = index of g among the valid groups in
 * FIRST-OCCURRENCE order (the row order of the reference's outputs, tf.unique :109) or -1.  The per-list sums (seg_lse, seg_ysum,
 * seg_psum, seg_pdot) are fp64: a row's gradient softmax_i * psum - p_i cancels where a list's one positive is its top logit, and
 * an fp32 log-sum-exp leaves such lists 1e-5 .. 1e-4 off relative to their own largest entry.
 * ---------------------------------------------------------------------------------------------------------- */
size_t recnow_listwise_workspace_bytes(int64_t B);
int recnow_listwise_segments(const float* labels, const float* logits, const int32_t* order, const int32_t* seg_first,
                             const int32_t* n_seg, int64_t B, float pos_neg_th, float pad_logit, int32_t* seg_valid,
                             double* seg_lse, double* seg_ysum, double* seg_psum, double* seg_pdot, int32_t* valid_rank,
                             int32_t* n_valid, void* ws, size_t ws_bytes, void* stream);
/* loss [1]; dbase[i] = w_g * (softmax_i * psum_g - p_i) (0 outside valid groups): d loss/d logits = dbase / n_valid
 * (do_reduce) or dbase * upstream[row_rank] (per-list losses);  row_rank[i] = valid rank of i's group or -1;
 * group_loss[r] = weighted loss of the r-th valid list.  weights: [n_valid] or NULL. */
int recnow_listwise_loss_fwdbwd(const float* labels, const float* logits, const int32_t* order, const int32_t* seg_id,
                                const int32_t* seg_first, const int32_t* seg_valid, const double* seg_lse,
                                const double* seg_ysum, const double* seg_psum, const double* seg_pdot,
                                const int32_t* valid_rank, const int32_t* n_valid, const float* weights, int64_t B,
                                float* loss, float* dbase, int32_t* row_rank, float* group_loss, void* stream);
/* to_listwise_sample + listwise_loss_via_softmax_cross_entropy_with_logits(do_reduce=True) fused on sorted segments, as ONE call
 * (rec_block/listwise_loss_from_batch.py:89-173): grouping of `groups` (one id tensor), the per-list statistics, the mean loss over
 * the valid lists (0 when there is none: nan_to_zero) and  dlogits[i] = d loss / d logits[i]  (already divided by the number of valid
 * lists), so that a host framework's backward is one multiply.  out2 (2 floats): {loss, (float) number of valid lists}.
 * weights: [>= number of valid lists] in first-occurrence order of the valid groups, or NULL.  One workspace
 * (recnow_listwise_loss_workspace_bytes) holds every intermediate.  key_dtype: RECNOW_KEY_INF_EQUAL is accepted and implied. */
size_t recnow_listwise_loss_workspace_bytes(int64_t B, int key_dtype);
int recnow_listwise_loss(const void* groups, int key_dtype, const float* labels, const float* logits, const float* weights, int64_t B,
                         float pos_neg_th, float pad_logit, float* out2, float* dlogits, void* ws, size_t ws_bytes, void* stream);
/* Dense (n_valid,B) outputs of to_listwise_sample (:131-148) for API parity.  The caller pre-fills mask_out = 0,
 * labels_out = 0, logits_out = pad_logit; members of valid groups are scattered in. */
int recnow_listwise_dense(const float* labels, const float* logits, const int32_t* order, const int32_t* seg_id,
                          const double* seg_ysum, const int32_t* valid_rank, int64_t B, uint8_t* mask_out,
                          float* labels_out, float* logits_out, void* stream);
int recnow_listwise_dense_bwd(const float* ddense, const int32_t* row_rank, int64_t B, float* dlogits, void* stream);
/* tf.nn.softmax_cross_entropy_with_logits over the rows of dense (G,N) matrices (:167): row_loss = lse*sum(p) - p.s;
 * backward dlogits[g][j] = grow[g] * (exp(s - lse_g) * psum_g - p).  HBM-bound streaming over G*N. */
int recnow_softmax_ce_rows_fwd(const float* labels, const float* logits, int64_t G, int64_t N, float* row_loss,
                               float* row_lse, float* row_psum, void* stream);
int recnow_softmax_ce_rows_bwd(const float* labels, const float* logits, const float* row_lse, const float* row_psum,
                               const float* grow, int64_t G, int64_t N, float* dlogits, void* stream);

/* In-batch ListMLE (ABI 23): the negative log-likelihood of the label-sorted permutation of every list under the Plackett-Luce model, on the
 * caller's sorted segments (order / seg_id / seg_first / n_seg of recnow_group_segments on the lists' keys).  The reference has no such loss.
 *   taking part   mask byte non-zero (mask may be NULL) and label not NaN; other rows get gradient 0 and influence nothing
 *   permutation   the taking-part rows of a list by label descending (-0.0 == +0.0), ties by ascending row index; n rows, logits s_1 .. s_n
 *   valid list    n >= 2 and at least two label values among the taking-part rows; valid lists are ranked by first occurrence in the batch
 *   K             n when topn == 0, else min(topn, n)
 *   list loss     l = sum_{p <= K} (lse_p - s_p), lse_p = log sum_{q >= p} exp(s_q); times 1 / K when list_mean; times weights[valid rank]
 *   gradient      dl/ds_q = exp(s_q + logA_q) - [q <= K], logA_q = log sum_{p <= min(q, K)} exp(-lse_p); same factors
 *   non-finite    a non-finite logit of a taking-part row makes its list's loss non-finite and its taking-part rows' gradients NaN, nothing else
 * Every output is optional (NULL):
 *   loss [1]        mean of the valid lists' losses, 0 when there is none          n_valid [1]   number of valid lists
 *   dbase [B]       per original row: d (list loss) / d logit, 0 outside valid lists; divided by n_valid when `reduce` != 0
 *   row_rank [B]    per original row: valid rank of its list, or -1                group_loss [B] per valid rank: the list's loss (first n_valid)
 *   position [B]    per original row: 0-based place in its list's permutation, -1 when it does not take part
 *   row_lse [B]     per original row: lse_p of its place, NaN when it does not take part
 *   list_loss [B], list_valid [B]   per SEGMENT (sorted numbering, first n_seg): l before 1 / K and weight; validity
 * weights: [B] readable entries, indexed by valid rank, or NULL.  The key words {seg_id, complement of the order-preserving image of the label}
 * are sorted by recnow_group_segments inside, on this entry's workspace; two fp64 segmented scans (logaddexp from each list's end, then from its
 * start) run over tiles of RECNOW_LISTMLE_TILE positions.  Where the caller's grouping or the inner one reported a grid-barrier time-out
 * (n_seg[0] < 0), loss, every entry of dbase and of group_loss are NaN and n_valid = -1.
 * RECNOW_EINVAL: B < 0, topn < 0, NULL order / seg_id / seg_first / n_seg / labels / logits / ws with B > 0; RECNOW_EWORKSPACE: ws_bytes below
 * recnow_listmle_workspace_bytes(B).  B == 0 writes loss = 0 and n_valid = 0.  No host synchronisation, no atomics, bitwise reproducible, every
 * launch can be captured in a HIP graph. */
#define RECNOW_LISTMLE_TILE 1024
size_t recnow_listmle_workspace_bytes(int64_t B);
int recnow_listmle_fwdbwd(const float* labels, const float* logits, const uint8_t* mask, const float* weights, const int32_t* order,
                          const int32_t* seg_id, const int32_t* seg_first, const int32_t* n_seg, int64_t B, int topn, int list_mean, int reduce,
                          float* loss, int32_t* n_valid, float* dbase, int32_t* row_rank, float* group_loss, int32_t* position, double* row_lse,
                          double* list_loss, int32_t* list_valid, void* ws, size_t ws_bytes, void* stream);

/* In-batch ApproxNDCG (ABI 24; Qin, Liu and Li 2010): a differentiable NDCG loss on the caller's sorted segments (order / seg_id / seg_first /
 * n_seg of recnow_group_segments), by two pair walks on the skeletons of the pairwise losses.  The reference has no such loss.
 *   lists and rows   a list is one segment; a row takes part when its mask byte is non-zero (mask may be NULL).  Rows that do not take part
 *                    influence nothing and get gradient exactly 0.
 *   temperature      tau, a finite float greater than 0
 *   soft position    R_i = sum_{j in the list, taking part, j != i} sigma((s_j - s_i) / tau), 0-based as D(r) = 1 / log2(2 + r)
 *   gain             G(y) = 2**y - 1 (RECNOW_NDCG_GAIN_EXP2) or y (RECNOW_NDCG_GAIN_LINEAR)
 *   ideal DCG        IDCG = sum G(y_i) D(q_i), q_i the label position of recnow_pair_lambda_terms (ties to the smaller original row index); no topn
 *   valid list       IDCG > 0 (a NaN label of a taking-part row makes the comparison false: the list is invalid)
 *   list loss        l = -ADCG / IDCG, ADCG = sum_i G(y_i) / log2(2 + R_i); the batch loss is the mean of l over the valid lists, 0 when none
 *   gradient         c_i = G(y_i) ln 2 / ((2 + R_i) ln^2(2 + R_i));  sigma'_kj = sigma(x) (1 - sigma(x)), x = (s_j - s_k) / tau;
 *                    dl/ds_k = (1 / (tau IDCG)) sum_{j != k, taking part} sigma'_kj (c_j - c_k); rows of an invalid list get exactly 0 (a select)
 *   NaN scores       a NaN score of a taking-part row makes its own list's loss NaN (and so the batch mean) and that list's taking-part rows'
 *                    gradients NaN; every other list's gradient bits stay as they were.  A row that does not take part may hold anything.
 * Every output is optional (NULL):
 *   loss [1]         float32 mean over the valid lists            loss_sum [1]   fp64 sum of l over the valid lists
 *   n_lists [1]      int64 number of valid lists                  dscores [B]    per original row: d loss / d score (already divided by n_lists)
 *   approx_rank [B]  fp64 per original row: R_i, NaN for a row that does not take part
 *   list_adcg [B], list_idcg [B]   fp64 per SEGMENT (sorted numbering, first n_seg)
 * float32 sigmoids from the hardware exp2 / rcp, the same bits for both rows of a pair; fp64 accumulators of R, fp64 per-row logarithms and
 * list sums in fixed order; no pair list, no float atomics, no host synchronisation, bitwise reproducible, capturable in a HIP graph.
 * Where the grouping reported a grid-barrier time-out (n_seg[0] < 0): loss, loss_sum and every entry of dscores NaN, n_lists = -1.
 * RECNOW_EINVAL: B < 0, an unknown gain, a temperature that is not finite and > 0, NULL scores / labels / order / seg_id / seg_first / n_seg /
 * ws with B > 0; RECNOW_EWORKSPACE: ws_bytes below recnow_approx_ndcg_workspace_bytes(B) (it begins with the pairwise workspace).  B == 0 writes
 * loss = 0, loss_sum = 0 and n_lists = 0. */
size_t recnow_approx_ndcg_workspace_bytes(int64_t B);
int recnow_approx_ndcg_fwdbwd(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order, const int32_t* seg_id,
                              const int32_t* seg_first, const int32_t* n_seg, int64_t B, int gain, float temperature, float* loss,
                              double* loss_sum, int64_t* n_lists, float* dscores, double* approx_rank, double* list_adcg, double* list_idcg,
                              void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * FMLayer: rec_now/layers/fm_layer.py:24-42.   HBM-bound (12*B*F*D bytes fwd+bwd).
 *   y[b] = 0.5 * sum_d [ (sum_f x_f[b][d])^2 - sum_f x_f[b][d]^2 ]
 * fields: DEVICE array of F device pointers, each a contiguous (B,D) fp32 tensor (the reference's list input);
 * y: [B]; S: [B*D] field sums saved for backward (NULL = forward only).
 * ---------------------------------------------------------------------------------------------------------- */
int recnow_fm_fwd(const float* const* fields, int F, int64_t B, int D, float* y, float* S, void* stream);
/* dfields[f][b][d] = gy[b] * (S[b][d] - x_f[b][d]);  dfields: DEVICE array of F device pointers to (B,D) buffers. */
int recnow_fm_bwd(const float* const* fields, float* const* dfields, int F, int64_t B, int D, const float* S,
                  const float* gy, void* stream);
/* Which kernel recnow_fm_fwd (which = 0) / recnow_fm_bwd (which = 1) launch for a call of this shape: the ONE statement of that choice (both
 * launchers call the function behind it); nothing is launched and no device is needed.  has_S: S != NULL (1 is required for the backward).
 * Returns family * 100000 + save_s * 1000 + lanes_per_row.  family: 1 k_fm_*_generic (lanes_per_row 0), 2 k_fm_*_vec4, 3 k_fm_*_wide;
 * save_s: the forward instantiation that writes S (0 for the backward); lanes_per_row = D / 4.  B = 0: 0 (no launch).  RECNOW_EINVAL: which
 * outside {0, 1}, F < 1, B < 0, D < 1, has_S outside {0, 1}, or the backward without S. */
int recnow_fm_route(int which, int64_t B, int F, int D, int has_S);

/* ------------------------------------------------------------------------------------------------------------
 * Exact-fp32 MFMA GEMM (v_mfma_f32_32x32x2_f32: every product/accumulate is an fp32 fma, no reduced precision),
 * the dense contraction under MultiDenseLayer (multi_dense_layer.py:90), DCNMixLayer (dcn_mix_layer.py:135-141),
 * MMOELayer / PLELayer experts and gates.  Bound: fp32 MFMA peak (157 TFLOP/s), not HBM.
 *     C[b] = epilogue( opA(A[b]) x opB(B[b]) ),   b = 0 .. batch-1
 *     epilogue(v) = act(v + bias[n]) * emul[m][n]  (+ C[m][n] when accumulate)
 * Operand modes fuse the elementwise producer of a gradient GEMM into the operand load:
 *     MUL:      operand[i] * second[i]                       ACTGRAD:  operand[i] * act'(second[i]), act' through the
 *                                                                      activation OUTPUT (1-y^2, y(1-y), y>0)
 * A batch stride of 0 broadcasts that operand.  K-splitting (deterministic slab reduce) is chosen internally when
 * M*N is small and K is large (weight gradients, K = batch rows).
 * ---------------------------------------------------------------------------------------------------------- */
#define RECNOW_OPMODE_NONE 0
#define RECNOW_OPMODE_MUL 1
#define RECNOW_OPMODE_ACTGRAD 2
#define RECNOW_OPMODE_OUTER 3   /* operand(row,col) = second[row][col / hq] * first[row][col % hq]: CIN's outer product
                                 (cin_layer.py:103) generated in the operand load; row = the operand's non-k index for A
                                 in [M][K] storage / B in [N][K] storage, and the k index for [K][M] / [K][N] storage */

typedef struct recnow_gemm_desc {
    const float* A;  const float* A2; int64_t lda; int64_t a_batch_stride; int a_trans; int a_mode; int a_act; int a_pad;
    const float* B;  const float* B2; int64_t ldb; int64_t b_batch_stride; int b_trans; int b_mode; int b_act; int b_pad;
    float* C; int64_t ldc; int64_t c_batch_stride;
    int M, N, K, batch;               /* logical A: (M,K), B: (K,N), C: (M,N) */
    const float* bias; int64_t bias_batch_stride;
    const float* emul; int64_t lde; int64_t e_batch_stride;
    int act;                          /* RECNOW_ACT_* applied to columns < act_cols (act_cols <= 0: all columns) */
    int act_cols;
    int e_mode; int e_act;            /* e_mode 0/MUL: v *= emul[m][n];  ACTGRAD: v *= act'(emul[m][n]) (e_act) */
    int accumulate;
    int a_hq; int b_hq;               /* OUTER mode: inner width hq (A2/B2 hold the [row][col / hq] factor) */
    int64_t a_ld2; int64_t b_ld2;     /* OUTER mode: row stride of A2 / B2 */
    int c_trans;                      /* 1: store the result transposed, C[n][m] (ldc = row stride of that layout) */
    /* Side product (lean 128x128 kernels, batch 1): sp_r <= 4 extra output columns computed on the VALU from the A tile
     * in LDS:  sp_cx[m*sp_cx_ms + r*sp_cx_rs] = sum_k A'[m][k] * sp_bx[k*sp_bx_ks + r*sp_bx_rs]  (A' = A after its
     * operand mode).  DCN-v2 uses it for the N gate columns so that N*S + N = 130 runs as exactly 128 MFMA columns. */
    const float* sp_bx; float* sp_cx; int64_t sp_bx_ks, sp_bx_rs, sp_cx_ms, sp_cx_rs; int sp_r; int sp_pad;
    /* Rank-R epilogue update (lean 128x128 kernels, batch 1): before bias-activation / emul,
     *   v[m][n] += sum_{r < eu_r <= 4} eu_p[m*eu_pms + r] * eu_q[r*eu_qrs + n*eu_qns]  (K = 128 + 2 as exactly 128).  Never split over K. */
    const float* eu_p; const float* eu_q; int64_t eu_pms, eu_qrs, eu_qns; int eu_r; int eu_pad;
    double prof_flops;                /* algorithmic flops of this product for the measurement hook (0: 2*M*N*K*batch);
                                         callers that zero-pad K or move columns to a side product state the true count */
    /* Second output of the same accumulators (short-K persistent kernel only: K <= 512, K % 16 == 0, M, N multiples of
     * 128, A [M][K], batch 1, no bias / activation / transposed store; anything else returns RECNOW_EUNSUPPORTED):
     *   c2_mode 1:  C2[m][n]  = acc                    (DCN-v2 forward keeps O next to y = x * O)
     *   c2_mode 2:  C2[m][n] += acc * E2[m][n]         (DCN-v2 backward: dx += g_l * O_l in the kernel that produces g_l)
     * `acc` is the raw product A B, before emul / accumulate are applied for C. */
    float* C2; int64_t ldc2; const float* E2; int64_t lde2; int c2_mode; int c2_pad;
    /* Elementwise side output of the A stream (lean 128x128 kernels with a side product, A [M][K], a_mode MUL, batch 1,
     * no split-K; written by the workgroups of the first column tile):
     *   as_out[m][k] = A[m][k] * as_in[m][k]      (both with A's leading dimension lda)
     * DCN-v2 backward: the dT2g product streams g = dL/dy anyway and writes dx = g * O on the way. */
    const float* as_in; float* as_out;
    /* More second-output forms of the short-K kernel (same shape rules as c2_mode 1 / 2), used by the model-level fused step
     * "cross layers + scoring head" (recnow_dcn_mix_score_fwd/bwd):
     *   c2_mode 3 (emul required, b_trans 0): C2 = acc; C = acc * emul is NOT stored; instead its row-dot with the column
     *              vector hv (N) leaves as partials hp[m * hp_ld + 2 * (n / 128) + ((n % 128) / 64)], hp_ld >= N / 64: a
     *              Dense(1) head folded into the epilogue of the product that forms its input.
     *   c2_mode 4 (b_trans 1, no emul): C = acc; C2[m][n] = acc * E2[m][n] + rv[m] * cv[n] * E3[m][n] (written, not read). */
    const float* E3; int64_t lde3; const float* rv; const float* cv; const float* hv; float* hp; int hp_ld; int hp_pad;
    /* k_valid (0 = K): the caller guarantees that A's columns / B's rows k_valid .. K-1 are ZERO (a depth padded to the k-tile);
     * the short-K kernel then skips the MFMA steps of the padding (DCN-v2: 130 of 144). */
    int k_valid; int k_pad;
    /* c_perm_s > 0 (split-K products only, batch 1, no transposed store / accumulate; else RECNOW_EINVAL / EUNSUPPORTED): the result
     * is stored as [N / c_perm_s][M][c_perm_s] instead of [M][N], C[((n / s) * M + m) * s + n % s] -- DCN-v2's dU (N, D, S) straight
     * from the product x_l^T dA (D x N*S), without an unpack pass. */
    int c_perm_s; int c_perm_pad;
    /* Fused sub-space forward of DCNMixLayer (rec_now/layers/dcn_mix_layer.py:135-138,146-147; lean 128x128 kernel, batch 1, no split-K):
     * the product is formulated TRANSPOSED -- A = [U | K]^T stored [K][M] with M = N_e * S = 128 (a_trans 1), B = x_l^T stored [N][K]
     * (b_trans 1), so "N" is the batch -- the side product (sp_bx = K, sp_r = 2) is taken from the B tile, and the epilogue continues
     * from the accumulators: H1 = act(acc) -> mid_T1 [row][s]; per expert C = H1 V on the MFMA with the accumulator registers as the A
     * fragments (k pairs (s, s + 4): no LDS round trip), H2 = mid_act_outer(C) -> mid_T2, G = softmax(logits), mid_T2g = [G * H2 | G | 0],
     * logits -> mid_T1[:, 128 + e].  mid_V (2, 64, 64); mid_T1 / mid_T2 / mid_T2g (N x mid_ld).  C is not written. */
    const float* mid_V; float* mid_T1; float* mid_T2; float* mid_T2g; int64_t mid_ld; int mid_act_outer; int mid_pad;
    /* c2_mode 5 / 6 (ABI 4; short-K kernel, K = 144, b_trans 1, no emul / accumulate; C2 unused): the LAST product of a backward pass writes the
     * whole input gradient in one go,
     *   C[m][n] = acc + E2 * E3 [+ E4 * E5] + rv[m] * cv[n] * E6          (elementwise products; c2_mode 6 leaves the bracket out)
     * all five tensors with the leading dimension lde2 (= lde3), every one read once, C written once and never read.  DCN-v2 (round 5): d loss / d x
     * = g_0 + g_1 * O_0 + g_2 * O_1 + dscore (x) w_head * O_2 is accumulated ONCE, by the product that forms g_0, instead of as a read-modify-write in
     * the product of every layer: 8 instead of 10 passes over a (B, D) tensor per step. */
    const float* E4; const float* E5; const float* E6;
    /* a_trans = 0: A stored [M][K] (lda = row stride);  1: stored [K][M]
     * b_trans = 0: B stored [K][N] (ldb = row stride);  1: stored [N][K] */
} recnow_gemm_desc;

size_t recnow_gemm_workspace_bytes(const recnow_gemm_desc* desc_host);
int recnow_gemm(const recnow_gemm_desc* desc_host, void* ws, size_t ws_bytes, void* stream);
/* Which kernel recnow_gemm(desc_host, ws, ws_bytes, stream) launches, with a non-NULL ws when ws_bytes > 0: the ONE statement of that choice
 * (recnow_gemm launches what the function behind it plans); host-only, nothing is launched and no pointer of the descriptor is dereferenced
 * (addresses are read for their alignment).  It uses the process's precision, staging and environment switches and returns what recnow_gemm
 * would return before its first launch; the fields are meaningful on RECNOW_OK (ABI 28).
 *   family   0 nothing to launch (M, N or batch is 0), 1 k_gemm, 2 k_gemm_shortk (fp32), 3 k_gemm_shortk on piece planes (K = 144),
 *            4 k_gemm_split, 5 k_gemm_s3
 *   bm, bn, bk, a_kc, b_kc, edge, a2k, b2k, xf   family 1: the template arguments of k_gemm<BM, BN, WM, WN, BK, A_KC, B_KC, EDGE, A2K, B2K, XF>
 *            (WM x WN waves: 2 x 2 for 128 x 128 and 64 x 128 tiles, else 4 x 1; A_KC: A stored [M][K]; B_KC: B stored [N][K]; the EDGE kernels
 *            take the operand modes at run time: a2k = b2k = -1).  Families 4 and 5: a_kc, b_kc, a2k of k_gemm_split<A_KC, A2K, BP> /
 *            k_gemm_s3<A_KC, A2K, PAIR>; bp: 0 B [K][N], 1 B [N][K], both split in the kernel, 2 B from piece planes; pair: paired A loads
 *   ep, c2_mode   families 2 and 3: ep = (emul ? 1 : 0) | (accumulate ? 2 : 0) and the second-output form
 *   planes   0 none; 1 B is split into piece planes in the workspace first (family 3: rn_split_planes at its base; 4, 5: k_split_planes behind
 *            the slabs); 2 planes the caller holds (internal callers only: never from this query)
 *   splitk, kchunk   K slices and their length (splitk > 1: slabs in the workspace and a reduction); grid_x, grid_y, grid_z: the product's grid
 *            (family 2 / 3: the tile counts, the persistent kernel sizes its own grid); xcd_remap 0 / 1 / 2; tail_pairs: k pairs of the last
 *            16-deep k-tile that k_valid leaves (8: all)
 *   reduce_variant, reduce_blocks   splitk > 1: k_gemm_splitk_reduce<VEC, QUAD> 0 <false, false>, 1 <true, false>, 2 <true, true> and its grid
 *   tag      the launch's recnow_prof tag (RN_TAG_GEMM_*, csrc/prof_tags.hpp): it names the kernel that runs */
typedef struct recnow_gemm_route_info {
    int32_t family, bm, bn, bk, a_kc, b_kc, edge, a2k, b2k, xf, bp, pair, ep, c2_mode, planes;
    int32_t splitk, kchunk, grid_x, grid_y, grid_z, xcd_remap, tail_pairs, reduce_variant, reduce_blocks, tag;
} recnow_gemm_route_info;
int recnow_gemm_route(const recnow_gemm_desc* desc_host, size_t ws_bytes, recnow_gemm_route_info* out);
/* Process-wide arithmetic of the long-K 128-column products with a side product (the K = 1024 / K = B products of DCNMixLayer):
 *   0 (default) exact fp32 MFMA -- an fp32 fma chain, what TF's fp32 matmul computes up to summation order;
 *   1 "bf16x3": every fp32 operand element split into three bf16 pieces, six bf16 MFMA terms per product, fp32 accumulation:
 *     relative error of a product <= 2^-25, results within the 1e-5 parity bound but NOT bit-identical to mode 0 (opt-in).
 *     Finite operands up to FLT_MAX give finite products (piece 1 saturates at +-bf16_max, pieces 2 and 3 carry the rest).  Non-finite
 *     operands give non-finite outputs where mode 0 does, but not always of the same class: an inf may come out as NaN.  Operands below
 *     2^-100, where pieces 2 and 3 become subnormal, are not verified.
 * Also read once from the environment (RECNOW_GEMM_PRECISION=bf16x3).  Shapes without a split kernel run mode 0 regardless. */
int recnow_set_gemm_precision(int mode);
int recnow_get_gemm_precision(void);
/* Process-wide operand staging of the long-K products whose two operands are plain [k][row] tensors (the K = B weight-gradient products dU_l of
 * DCNMixLayer): 0 (default) global -> registers -> LDS, 1 LDS-DMA (global_load_lds_dwordx4, no staging registers).  Same LDS image, same k order:
 * the results are bit-identical; kept as an A/B switch (profiles/r05_glds_ab.md: neutral).  Also read once from RECNOW_GEMM_GLDS=1.  Returns RECNOW_OK. */
int recnow_set_gemm_staging(int mode);
int recnow_get_gemm_staging(void);

/* ------------------------------------------------------------------------------------------------------------
 * MultiDenseLayer: rec_now/layers/multi_dense_layer.py:80-94.   y[n] = act(x[n] @ kernel[n] + bias[n])
 *   x: (B,D) when x_batched == 0 (broadcast to every n, :88-89) else (N,B,D); kernel (N,D,U); bias (N,1,U) or NULL;
 *   y: (N,B,U).  act must be a RECNOW_ACT_* code (other activations are applied by the caller on the linear output).
 * Backward (derived from the forward lines; the reference leaves it to TF autodiff):
 *   dZ = dy * act'(y);  dkernel[n] = x[n]^T dZ[n];  dbias[n] = colsum dZ[n];  dx[n] = dZ[n] kernel[n]^T (summed over n
 *   when x was broadcast).  Any of dx / dkernel / dbias may be NULL (not needed).
 * ---------------------------------------------------------------------------------------------------------- */
size_t recnow_multi_dense_workspace_bytes(int64_t B, int D, int U, int N);
int recnow_multi_dense_fwd(const float* x, int x_batched, const float* kernel, const float* bias, int64_t B, int D, int U,
                           int N, int act, float* y, void* ws, size_t ws_bytes, void* stream);
int recnow_multi_dense_bwd(const float* x, int x_batched, const float* kernel, const float* y, const float* dy, int64_t B,
                           int D, int U, int N, int act, float* dx, float* dkernel, float* dbias, void* ws, size_t ws_bytes,
                           void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Gate mixing of MMOELayer (mmoe_layer.py:109-117) and PLELayer (ple_layer.py:274-293):
 *   g[t][b][:] = softmax(logits[t][b][:]);   out[t][b][:] = sum_n g[t][b][n] * E_n[b][:]
 * experts: DEVICE array of N device pointers, expert n is a contiguous (B,U) matrix (so PLE's "own + shared" expert
 * subsets need no concat copy).  logits, gates: (T,B,N); out: (T,B,U).  HBM-bound.
 * Backward: dexperts[n] (+)= sum_t g*dout;  dlogits = g * (dg - sum_n g*dg), dg[t][b][n] = dout[t][b][:] . E_n[b][:].
 * accumulate_dexperts != 0 adds into dexperts (an expert feeding several gates).
 * ---------------------------------------------------------------------------------------------------------- */
int recnow_moe_mix_fwd(const float* logits, const float* const* experts, int T, int64_t B, int N, int U, float* gates,
                       float* out, void* stream);
int recnow_moe_mix_bwd(const float* gates, const float* const* experts, const float* dout, int T, int64_t B, int N, int U,
                       float* dlogits, float* const* dexperts, int accumulate_dexperts, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * DCNLayer (DCN-v1 cross, reference variant without residual): rec_now/layers/dcn_layer.py:79-103
 *   x_{l+1} = act(x0 * (x_l . w_l) + b_l),  l = 0..L-1;  all L layers fused in one pass over x0 (HBM-bound: 8*B*D
 *   bytes forward, 20*B*D backward incl. the recompute read).  Any L, any D, any alignment: the fused register kernels
 *   cover L <= 4 and D <= 4096 (D % 4 == 0, 16-byte aligned rows; else D <= 1024); other shapes run the same math as
 *   streaming kernels over the per-row scalars (rows kernel + columns kernel, see csrc/dcn.hip).
 *   kernels: (L,D) (row l = kernel_l[:,0]); biases: (L,D) or NULL (use_bias=False); y: (B,D).
 *   csave: optional (B,L) output of the forward, the per-row scalars c_l = x_l . w_l.  Given to the backward, x_l is
 *   elementwise in x0 (one dot-reduce per layer, a wave per row); csave == NULL: the backward recomputes the forward per row
 *   from x0 (nothing saved).  dx (B,D), dkernels (L,D), dbiases (L,D) or NULL.
 * ---------------------------------------------------------------------------------------------------------- */
size_t recnow_dcn_workspace_bytes(int64_t B, int D, int L);
int recnow_dcn_fwd(const float* x, const float* kernels, const float* biases, int64_t B, int D, int L, int act, float* y,
                   float* csave, void* stream);
int recnow_dcn_bwd(const float* x, const float* kernels, const float* biases, const float* dy, const float* csave, int64_t B,
                   int D, int L, int act, float* dx, float* dkernels, float* dbiases, void* ws, size_t ws_bytes, void* stream);
/* One cross layer with its own layer input (one iteration of the loop at rec_now/layers/dcn_layer.py:91-100):
 *   z = act(x0 * (x_l . w) + b);  c_out (B) = x_l . w is kept for the backward.  Used when the activation between the layers
 *   is a user callable (keras.activations.get accepts any, dcn_layer.py:30 via keras.layers.Dense): act = RECNOW_ACT_LINEAR
 *   here and the callable runs on z.  Any D, any alignment.  w, b: (D); b may be NULL.
 *   backward: dz is the gradient w.r.t. z; z may be NULL when act is linear.  dx0, dxl (B,D) are written (not accumulated);
 *   dw (D), db (D, may be NULL). */
size_t recnow_dcn_step_workspace_bytes(int64_t B, int D);
int recnow_dcn_step_fwd(const float* x0, const float* xl, const float* w, const float* b, int64_t B, int D, int act, float* z,
                        float* c_out, void* stream);
int recnow_dcn_step_bwd(const float* x0, const float* xl, const float* w, const float* z, const float* c, const float* dz,
                        int64_t B, int D, int act, float* dx0, float* dxl, float* dw, float* db, void* ws, size_t ws_bytes,
                        void* stream);
/* Which kernels recnow_dcn_fwd (which = 0) / recnow_dcn_bwd (which = 1) launch for a call of this shape: the ONE statement of that choice (both
 * drivers call the function behind it); nothing is launched.  has_csave: csave != NULL (it moves the backward only).  align_mask: one bit per
 * tensor that starts OFF a 16-byte boundary -- 1 x, 2 y (forward) / dy (backward), 4 dx (backward), 8 kernels, 16 biases (NULL: clear).
 * Returns family * 100000 + tpr * 100 + vec * 10 + nv, (tpr, vec, nv) the threads per row, floats per access and register images per thread of
 * the kernel template (0, 0, 0 on the general path).  family, forward: 1 k_dcn_fwd_general, 2 k_dcn_fwd, 3 k_dcn_fwd_fast; backward: 1 the
 * general rows + columns kernels, 2 k_dcn_bwd (recompute, no csave), 3 k_dcn_bwd_saved, 4 k_dcn_bwd_saved_wl, 5 k_dcn_bwd_fast.  B = 0: 0 (no
 * launch).  RECNOW_EINVAL: which outside {0, 1}, B < 0, D < 1, L < 1 or align_mask outside 0 .. 31. */
int recnow_dcn_route(int which, int64_t B, int D, int L, int has_csave, int align_mask);

/* ------------------------------------------------------------------------------------------------------------
 * DCNMixLayer (DCN-v2 mixture of low-rank experts, reference variant without residual):
 * rec_now/layers/dcn_mix_layer.py:114-151.  Per layer l (x_0 = x):
 *   A = x_l U_n -> act_inner -> (. V_n) -> act_outer -> (. W_n + b_n) -> * x   ;   gates = softmax(x_l K)
 *   x_{l+1} = sum_n gates[:,n] * (...)_n
 * Weight pointer arrays are HOST arrays of L DEVICE pointers:
 *   U[l]: (N,D,S) origin_to_sub_kernels_of_layer{l};  V[l]: (N,S,S) sub_to_sub_...;  W[l]: (N,S,D) sub_to_origin_...;
 *   bias[l]: (1,N,D) bias_of_layer{l};  gate[l]: (D,N) gate_of_layer{l} kernel (Dense, use_bias=False).
 * The two D-sized contractions per layer run on the exact-fp32 MFMA GEMM with the gate logits folded in as extra
 * columns and the gate-weighted bias folded in as extra K rows; `saved` keeps the small (B x ~(N*S+N)) activations
 * and the layer inputs for backward.
 * What `saved` holds depends on the route its forward took, and the note below records it: per layer T1 / T2 / T2g; the layer outputs x_{l+1}
 * or (when they are not materialised) nothing in their place; O_l = T2g_l [W; b] per layer; the packed weights and their piece planes.  A fused-head
 * forward in split-precision mode on the launch-per-product route ("head-Q", csrc/dcnmix.hip) takes the score as the row dot T2g_{L-1} . Q with
 * Q = x (W_{L-1} * head_w)^T: it keeps Q (B x ~(N*S+N)) where x_1 would sit, writes NO O_{L-1}, and leaves the planes of [W; b]_{L-1} * head_w where
 * those of [W; b]_{L-1} would be.  Its backward reads Q as the head's dT2g; one that cannot run the matching input-gradient form (precision flipped
 * since) recomputes O_{L-1} first.  Sizes are the same on every route (tests/golden/dcn_mix_sizes.npz).
 *
 * Library state (the whole of it).
 *   - Process-wide settings: recnow_set_gemm_precision, recnow_set_gemm_staging, recnow_prof_* (one launching thread per process is the model).
 *   - One host-side NOTE per `saved` buffer of the DCN-v2 entries, keyed by the buffer's ADDRESS (a table of 256 entries under a mutex,
 *     csrc/dcnmix.hip): which weight packs / piece planes the forward that filled it left there, because the route rule (batch size,
 *     precision mode, RECNOW_TILE) is read per call and may differ between a forward and its backward.  Contract: every forward call
 *     (recnow_dcn_mix_fwd / _score_fwd / the FORWARD phase of recnow_dcn_mix_step) RE-WRITES the note of its `saved` before any backward can read
 *     it, so a recycled address -- another shape, another allocation -- never meets a stale note; a backward whose `saved` has no note (filled
 *     by another copy of the library, or more than 256 distinct buffers ago) packs what its route needs itself: slower by one pack launch,
 *     never wrong.  The note holds no device data and no pointer is dereferenced through it.
 *   - Thread-local hand-offs between the phases of ONE recnow_dcn_mix_step call (packs written by the GROUP phase's front kernel, the piece
 *     planes of the next product): consumed inside the call that set them.
 * ---------------------------------------------------------------------------------------------------------- */
size_t recnow_dcn_mix_saved_bytes(int64_t B, int D, int S, int N, int L);
size_t recnow_dcn_mix_workspace_bytes(int64_t B, int D, int S, int N, int L);
int recnow_dcn_mix_fwd(const float* x, const float* const* U_host, const float* const* V_host, const float* const* W_host,
                       const float* const* bias_host, const float* const* gate_host, int64_t B, int D, int S, int N, int L,
                       int act_inner, int act_outer, float* y, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                       void* stream, int need_dx);
/* need_dx: 0 when the caller will not ask for the gradient w.r.t. x (x is data, as under tf.GradientTape.gradient(loss,
 * weights)): the forward then keeps nothing that only dx needs.  recnow_dcn_mix_bwd must be given dx == NULL after such a
 * forward, and may be given dx == NULL after any forward: the products and passes that only feed dx are not launched. */
int recnow_dcn_mix_bwd(const float* x, const float* const* U_host, const float* const* V_host, const float* const* W_host,
                       const float* const* bias_host, const float* const* gate_host, const float* dy, const void* saved,
                       size_t saved_bytes, int64_t B, int D, int S, int N, int L, int act_inner, int act_outer, float* dx,
                       float* const* dU_host, float* const* dV_host, float* const* dW_host, float* const* dbias_host,
                       float* const* dgate_host, void* ws, size_t ws_bytes, void* stream, void* stream2);

/* Model-level fusion of the north-star step: the L cross layers followed by a Dense(1) scoring head,
 *   scores[m] = DCNMix(x)[m] . head_w + head_b        (rec_now/layers/dcn_mix_layer.py:149-150 -> multi_dense_layer.py:90-92
 *                                                       with units = 1, num_dnn = 1)
 * The head is folded into the epilogue of the last layer's output product (the layer output is never stored) and its rank-one
 * gradient dscore (x) head_w is never materialised in the backward (see csrc/dcnmix.hip).  Same saved / workspace sizes as
 * recnow_dcn_mix_fwd/bwd.  recnow_dcn_mix_score_supported: 1 when the shape takes the fused route (N*S and D multiples of 128,
 * B a multiple of 256, S in {32, 64}, L <= 8), else 0 -- the caller then composes recnow_dcn_mix_* with recnow_multi_dense_*.
 * head_w (D), head_b (1) or NULL, scores (B), dscores (B), dhead_w (D), dhead_b (1) or NULL.
 * layer_events_host: optional HOST array of L hipEvent_t (entries may be NULL): event l is recorded when every weight gradient
 * of layer l has been issued (layers are walked L-1 .. 0; the head's gradients are complete at event L-1), so a data-parallel
 * caller can all-reduce a layer's gradients while the lower layers' backward still runs. */
int recnow_dcn_mix_score_supported(int64_t B, int D, int S, int N, int L);
/* 1 when a step / score / layer call of this shape runs the row-block persistent kernels (csrc/dcnmix_tile.hip: two experts of 64,
 * D in {256, 512, 1024}, batches up to 16 384 rows; RECNOW_TILE=0 / =1 and the precision mode are read at every call): the ONE
 * statement of that rule -- callers that place other work around the cross layers (rec_now_amd/step.py: where the grouping of the
 * batch runs) ask here instead of restating it.  2 (round 6): split-precision mode with the FORWARD pass of all cross layers as one
 * row-block launch on the bf16 MFMA (csrc/dcnmix_tile_split.hip; RECNOW_TILE_SPLIT=0 / =1) and the backward pass one launch per product. */
int recnow_dcn_mix_tile_route(int64_t B, int D, int S, int N, int L);
int recnow_dcn_mix_score_fwd(const float* x, const float* const* U_host, const float* const* V_host, const float* const* W_host,
                             const float* const* bias_host, const float* const* gate_host, const float* head_w, const float* head_b,
                             int64_t B, int D, int S, int N, int L, int act_inner, int act_outer, float* scores, void* saved,
                             size_t saved_bytes, void* ws, size_t ws_bytes, void* stream, int need_dx);
int recnow_dcn_mix_score_bwd(const float* x, const float* const* U_host, const float* const* V_host, const float* const* W_host,
                             const float* const* bias_host, const float* const* gate_host, const float* head_w, const float* dscores,
                             const void* saved, size_t saved_bytes, int64_t B, int D, int S, int N, int L, int act_inner,
                             int act_outer, float* dx, float* const* dU_host, float* const* dV_host, float* const* dW_host,
                             float* const* dbias_host, float* const* dgate_host, float* dhead_w, float* dhead_b, void* ws,
                             size_t ws_bytes, void* stream, void* stream2, void* const* layer_events_host);
/* stream2: optional second hipStream_t (NULL or == stream: single-stream).  When given, the weight-gradient products and
 * the dx recompute run on it concurrently with the data-gradient chain on `stream`, ordered by events created and
 * destroyed inside the call; on return all of stream2's work is ordered before later work submitted to `stream`. */

/* The whole north-star step -- x -> L cross layers -> Dense(1) head -> in-batch pairwise (BPR) loss -> every gradient -- enqueued by
 * ONE call per phase, on buffers the caller allocates once (at 8192 rows per GPU, the 8-GPU shard of the metric's batch,
 * the ~60 launches of a step take less GPU time than a host framework needs to enqueue them one by one; a phase is one call, and,
 * because nothing is allocated and no event of the library is recorded inside, each phase can be captured into a HIP graph and
 * replayed).  Reference path: rec_now/layers/dcn_mix_layer.py:114-151 -> multi_dense_layer.py:80-94 ->
 * rec_block/pairwise_loss_from_batch.py:228-279 (pairloss_func = bpr_loss_func, no occurrence weights, optional mask).
 *
 * phases (bit mask, executed in this order within one call):
 *   RECNOW_STEP_GROUP     canonical keys + radix sort + segments of `groups` (score independent: may run on another stream,
 *                         under the forward pass; order it before RECNOW_STEP_LOSS with an event);
 *   RECNOW_STEP_FORWARD   recnow_dcn_mix_score_fwd -> scores;
 *   RECNOW_STEP_LOSS      loss, n_pair, stats, d loss / d scores (normalised by 1 / (P + 1e-10) when reduce_mean, else the
 *                         gradient of the loss SUM: a data-parallel caller divides by the global pair count after its all-reduce);
 *   RECNOW_STEP_BACKWARD  recnow_dcn_mix_score_bwd for the cross layers layer_hi .. layer_lo (descending; the head's gradients
 *                         belong to layer L-1).  A caller that all-reduces per layer issues one call (one graph) per layer.
 * All of a step's phases must use the same descriptor contents and workspace.  Shapes: recnow_dcn_mix_score_supported.
 * Any split of the phases over calls gives the same results; GROUP | FORWARD | LOSS in ONE call is the cheapest form at shard sizes (round 5): the
 * grouping launch then also writes the row-block kernels' weight packs on its spare workgroups and clears the pair counter, and the pair walk
 * fills its LDS stages straight from scores / labels / mask (no pack launch, no fill). */
#define RECNOW_STEP_GROUP 1
#define RECNOW_STEP_FORWARD 2
#define RECNOW_STEP_LOSS 4
#define RECNOW_STEP_BACKWARD 8
typedef struct recnow_dcn_mix_step_desc {
    int64_t B;
    int D, S, N, L;
    int act_inner, act_outer;           /* RECNOW_ACT_* of the cross layers */
    int group_dtype;                    /* RECNOW_KEY_* of `groups` */
    int only_use_wrong_order_pair;      /* pairwise_loss(only_use_wrong_order_pair=...) */
    int reduce_mean;                    /* 1: loss = sum / (P + 1e-10) (the reference's), 0: the sum */
    float factor;                       /* bpr_loss_func(factor=...) */
    const float* x;                     /* (B, D) */
    const float* labels;                /* (B) */
    const void* groups;                 /* (B) ids */
    const uint8_t* mask;                /* (B) or NULL */
    const float* const* U_host;         /* HOST arrays of L DEVICE pointers, as recnow_dcn_mix_fwd */
    const float* const* V_host;
    const float* const* W_host;
    const float* const* bias_host;
    const float* const* gate_host;
    const float* head_w;                /* (D) */
    const float* head_b;                /* (1) or NULL */
    float* scores;                      /* out (B) */
    float* loss;                        /* out (1) */
    int64_t* n_pair;                    /* out (1) */
    float* stats;                       /* out (2) or NULL: {loss as stored, (float) n_pair}, e.g. the tail of a gradient bucket */
    float* dx;                          /* out (B, D) or NULL: x is data */
    float* const* dU_host;              /* HOST arrays of L DEVICE pointers: the gradients */
    float* const* dV_host;
    float* const* dW_host;
    float* const* dbias_host;
    float* const* dgate_host;
    float* dhead_w;                     /* out (D) */
    float* dhead_b;                     /* out (1) or NULL */
    void* ws;                           /* recnow_dcn_mix_step_workspace_bytes; holds the step's state between the phases */
    size_t ws_bytes;
    void* stream2;                      /* optional second hipStream_t of RECNOW_STEP_BACKWARD (as recnow_dcn_mix_score_bwd's stream2): the
                                           weight-gradient products run on it beside the data-gradient chain; NULL: one stream */
    void* const* layer_events_host;     /* optional HOST array of L hipEvent_t (entries may be NULL), as recnow_dcn_mix_score_bwd: event l is
                                           recorded once every weight gradient of layer l has been issued.  Must be NULL while the call
                                           is being captured into a graph (an event recorded inside a capture belongs to the graph). */
    int64_t B_pad;                      /* 0 or == B: every buffer has B rows.  > B (ABI 4): RAGGED batch on the fast route -- the per-rank
                                           batches of whole groups that data parallelism produces (rec_now_amd/dp.py shard_rows_by_group)
                                           are not multiples of 256.  x, dx and scores then have B_pad rows of storage, B_pad a multiple of
                                           256 that recnow_dcn_mix_score_supported accepts; rows [B, B_pad) of x must be ZERO (written once
                                           by the caller); the layers run over B_pad rows, the grouping and the loss over the first B
                                           (labels, groups, mask: B elements), d loss / d scores of the padding rows is zero, so they add
                                           exactly 0.0f to every gradient; scores[B..B_pad) = head_b and dx rows >= B = 0 are written.
                                           Workspace: recnow_dcn_mix_step_workspace_bytes(B_pad, ...). */
} recnow_dcn_mix_step_desc;
size_t recnow_dcn_mix_step_workspace_bytes(int64_t B, int D, int S, int N, int L, int group_dtype);
int recnow_dcn_mix_step(const recnow_dcn_mix_step_desc* desc_host, int phases, int layer_hi, int layer_lo, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * CINLayer (xDeepFM Compressed Interaction Network): rec_now/layers/cin_layer.py:72-122
 *   X_k[b,d,c] = sum_{f,h} W_k[c, f*H_{k-1}+h] * x0[b,d,f] * X_{k-1}[b,d,h]   (X_0 = x0, H_0 = F)          (:103-109)
 *   out = sum over the channels of all kept layers -> (B,D)            (sum_channel, :116-117)
 *       | concat of the kept layers' channels, transposed -> (B, ctot*D) (:119-121); kept = [x0,] X_1..X_L (:112-113)
 * emb: (B, F*D) (concat of the field embeddings, :88-91); weights_host: HOST array of L DEVICE pointers, W_k stored
 * (H_k, F*H_{k-1}) = weight_of_layer{k}[0,0]; hidden_host: HOST int[L].  An implicit GEMM over M = B*D rows on the
 * exact-fp32 MFMA kernel; the (B,D,F,H) outer product is generated in the operand load and never stored.
 * `saved` keeps x0 transposed and X_1..X_L for backward.
 * ---------------------------------------------------------------------------------------------------------- */
size_t recnow_cin_saved_bytes(int64_t B, int D, int F, const int* hidden_host, int L);
size_t recnow_cin_workspace_bytes(int64_t B, int D, int F, const int* hidden_host, int L);
int recnow_cin_fwd(const float* emb, const float* const* weights_host, int64_t B, int D, int F, const int* hidden_host, int L,
                   int output_input, int sum_channel, float* out, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                   void* stream);
int recnow_cin_bwd(const float* const* weights_host, const float* dout, const void* saved, size_t saved_bytes, int64_t B, int D,
                   int F, const int* hidden_host, int L, int output_input, int sum_channel, float* demb,
                   float* const* dweights_host, void* ws, size_t ws_bytes, void* stream);

/* ============================================================================================================
 * SURVEY.md section 8f rows (neighbours of the hot path).
 * ========================================================================================================== */

/* InnerPNNLayer: rec_now/layers/inner_pnn_layer.py:25-53.  out[b][p] = <x_r[b], x_c[b]> over the F(F-1)/2 field pairs
 * r < c in r-major order (:41-45).  fields / dfields: DEVICE arrays of F device pointers to contiguous (B,D) fp32
 * tensors (the reference's list input); out, dout: (B, F(F-1)/2).  D <= 64.
 * Backward: dx_f[b][:] = sum_{g != f} dout[b][p(f,g)] * x_g[b][:]. */
int recnow_inner_pnn_fwd(const float* const* fields, int F, int64_t B, int D, float* out, void* stream);
int recnow_inner_pnn_bwd(const float* const* fields, float* const* dfields, int F, int64_t B, int D, const float* dout,
                         void* stream);
/* Which kernel recnow_inner_pnn_fwd (which = 0) / _bwd (which = 1) launch (the launchers call the function behind it; no launch, no device).
 * align_mask: 1 when `out` (forward) / `dout` (backward) starts OFF a 16-byte boundary.  Returns
 *   100000 + DMAX * 10 + waves                               k_ipnn_fwd / k_ipnn_bwd<DMAX> with `waves` waves per workgroup
 *   200000 + D * 100 + two * 10 + vec                        k_ipnn_fwd_gram<D>; two: F > 32; vec: float4 stores of the results
 *   300000 + D * 1000 + NB * 100 + FULL * 10 + vec           k_ipnn_bwd_gram<D, NB, FULL>; vec: float4 loads of dout
 * 0 for an empty call (B = 0; the forward with F = 1); RECNOW_EUNSUPPORTED where the launcher answers that (D > 64, or one row's tile does not
 * fit in LDS); RECNOW_EINVAL: which outside {0, 1}, F < 1, B < 0, D < 1, align_mask outside {0, 1}. */
int recnow_inner_pnn_route(int which, int64_t B, int F, int D, int align_mask);

/* SENETLayer: rec_now/layers/senet_layer.py:93-119.  Fields may have different widths: dims[f], offs[f] (first column of
 * field f in the concatenation, total = sum dims) are DEVICE int32 arrays.
 *   squeeze (:104-110):      sq[b][f] = mean_d x_f[b][d]                                  sq: (B,F)
 *   scale   (:112-117):      out[b][offs[f]+d] = x_f[b][d] * w[b][f]                      w: (B,F) excitation, out: (B,total)
 *   scale_bwd_w:             dw[b][f] = sum_d dout[b][offs[f]+d] * x_f[b][d]
 *   scale_bwd_x:             dx_f[b][d] = dout[b][offs[f]+d] * w[b][f] + dsq[b][f] / dims[f]   (dsq = gradient w.r.t. sq)
 * uniform_d > 0: the caller's promise that every field is uniform_d wide and all tensors are 16-byte aligned (selects the
 * float4 path when uniform_d/4 is a power of two); 0: general widths, staged through LDS (one concatenated row must fit:
 * total <= 12287).
 * The two Dense layers between squeeze and scale (:46-66) are recnow_multi_dense_* with N = 1. */
int recnow_senet_squeeze(const float* const* fields, const int32_t* dims, const int32_t* offs, int F, int total, int64_t B,
                         float* sq, int uniform_d, void* stream);
int recnow_senet_scale_fwd(const float* const* fields, const int32_t* dims, const int32_t* offs, int F, int total, int64_t B,
                           const float* w, float* out, int uniform_d, void* stream);
int recnow_senet_scale_bwd_w(const float* const* fields, const int32_t* dims, const int32_t* offs, int F, int total, int64_t B,
                             const float* dout, float* dw, int uniform_d, void* stream);
int recnow_senet_scale_bwd_x(float* const* dfields, const int32_t* dims, const int32_t* offs, int F, int total, int64_t B,
                             const float* w, const float* dout, const float* dsq, int uniform_d, void* stream);
/* The kernel the four entries above run for (B, F, total, uniform_d); mode 0 squeeze, 1 scale_fwd, 2 scale_bwd_w, 3 scale_bwd_x (all four choose
 * alike).  Host only: nothing is launched, no device memory is touched; the launchers run the very plan these report.
 *   recnow_senet_route: 0 nothing to do (B = 0); 100000 + R the LDS tile kernel on R rows per workgroup (1 .. 32); 200000 + Q the float4 kernel
 *   with Q = uniform_d / 4 lanes per field row; RECNOW_EUNSUPPORTED one concatenated row does not fit in LDS (total > 12287, not uniform);
 *   RECNOW_EINVAL mode outside 0 .. 3, F < 1, B < 0, total < 1, uniform_d < 0.
 *   recnow_senet_grid: the workgroups of that launch (the route's code where that is <= 0). */
int recnow_senet_route(int mode, int64_t B, int F, int total, int uniform_d);
int recnow_senet_grid(int mode, int64_t B, int F, int total, int uniform_d);

/* SENETLayer in one pass per direction (senet_layer.py:93-119), for equal field widths D (D % 4 == 0, D/4 a power of two,
 * F*D/4 <= 256), F <= 64, hidden width M <= 64 and RECNOW_ACT_* activations: squeeze, the F -> M -> F excitation and the
 * scaling read the fields once.  W1 (F,M), b1 (M), W2 (M,F), b2 (F) row-major (b1 / b2 may be NULL).
 *   fwd: out (B, F*D); saves sq (B,F), h (B,M) = act1(sq W1 + b1), w (B,F) = act2(h W2 + b2) for the backward pass.
 *   bwd: dfields[f] (B,D), dW1, db1, dW2, db2 (db1 / db2 may be NULL); deterministic (fixed-order partial sums).
 * recnow_senet_fused_supported returns 1 when (F, D, M) is inside these limits. */
int recnow_senet_fused_supported(int F, int D, int M);
size_t recnow_senet_fused_workspace_bytes(int64_t B, int F, int M);
int recnow_senet_fused_fwd(const float* const* fields, int F, int D, int64_t B, const float* W1, const float* b1, const float* W2,
                           const float* b2, int M, int act1, int act2, float* out, float* sq_save, float* h_save, float* w_save,
                           void* stream);
int recnow_senet_fused_bwd(const float* const* fields, float* const* dfields, int F, int D, int64_t B, const float* W1,
                           const float* W2, int M, int act1, int act2, const float* dout, const float* sq_save,
                           const float* h_save, const float* w_save, float* dW1, float* db1, float* dW2, float* db2, void* ws,
                           size_t ws_bytes, void* stream);
/* The kernel recnow_senet_fused_fwd (which = 0) / _bwd (which = 1) runs; out_misaligned: `out` is not on a 16-byte boundary (forward only).  The
 * launchers run the very plan these report.
 *   recnow_senet_fused_route: 0 nothing to do (B = 0); forward 100000 (4 rows per step) or 200000 (8 rows per step: D = 16, F % 8 == 0, out
 *   aligned) + 10 P + grant, P the threads that share one hidden unit (1, 2, 4, 8), grant 1 when the launch needs more than 64 KiB of LDS;
 *   backward 300000 + NACC, the instantiation (3, 5, 9, 17, 34 weight-gradient outputs per thread); RECNOW_EUNSUPPORTED outside
 *   recnow_senet_fused_supported; RECNOW_EINVAL which / out_misaligned outside {0, 1}, B < 0.  Launches nothing, touches no device memory.
 *   recnow_senet_fused_grid: the workgroups of that launch (the route's code where that is <= 0); the backward's follows the occupancy the
 *   runtime reports for the instantiation (at most 256 x occupancy workgroups), so it needs a device. */
int recnow_senet_fused_route(int which, int64_t B, int F, int D, int M, int out_misaligned);
int recnow_senet_fused_grid(int which, int64_t B, int F, int D, int M, int out_misaligned);

/* attention_by_dot_product: rec_now/rec_block/attention.py:12-38.  user (B,L,D), doc (B,D), D <= 256:
 *   s_l = <user[b][l], doc[b]> (max(.,0) when filter_neg, :31-32);  mat[b] = sum_l user[b][l] * s_l;  score_sum[b] = sum_l s_l
 * Backward recomputes s; dmat (B,D) / dsum (B) may be NULL (no gradient from that output). */
int recnow_attention_dot_fwd(const float* user, const float* doc, int64_t B, int L, int D, int filter_neg, float* mat,
                             float* score_sum, void* stream);
int recnow_attention_dot_bwd(const float* user, const float* doc, const float* dmat, const float* dsum, int64_t B, int L,
                             int D, int filter_neg, float* duser, float* ddoc, void* stream);
/* Which kernel recnow_attention_dot_fwd (which = 0) / _bwd (which = 1) launch (the launchers call the function behind it; no launch, no
 * device).  align_mask: one bit per tensor that starts OFF a 16-byte boundary (NULL is aligned) -- 1 user, 2 doc, 4 mat (forward) / dmat
 * (backward), 8 duser, 16 ddoc (backward only).  Returns 200000 + CPL for k_attn_dot_v4<CPL, ..> (CPL = D / 4), 100000 + GS for
 * k_attn_dot_fwd / _bwd<GS>; 0 for B = 0; RECNOW_EUNSUPPORTED for D > 256; RECNOW_EINVAL: which outside {0, 1}, B < 0, L < 0, D < 1,
 * align_mask outside 0 .. 7 (forward) / 0 .. 31 (backward). */
int recnow_attention_dot_route(int which, int64_t B, int L, int D, int align_mask);

/* attention_by_dnn (DIN attention unit, ABI 8): rec_now/rec_block/attention.py:41-82.  user (B,L,D), doc (B,D), nl Dense
 * layers of widths dims_host[0..nl) (a HOST array; dims_host[nl-1] must be 1), kernels_host / biases_host: HOST arrays of nl
 * DEVICE pointers, kernel 0 (2D, dims[0]) with the user rows first, kernel i (dims[i-1], dims[i]), row-major (Keras (in, out));
 * every bias present.  act (RECNOW_ACT_*) on all Dense layers but the last:
 *   logit[b,l] = Dense stack([user[b,l] | doc[b]]),  s = sigmoid(logit),  mat[b] = sum_l s user[b,l],  score_sum[b] = sum_l s
 * No (B,L,H) or (B,L,2D) tensor is formed.  Backward recomputes s; dmat (B,D) / dsum (B) may be NULL (no gradient from that
 * output); duser, ddoc required; dkernels_host / dbiases_host (HOST arrays of nl DEVICE pointers) may be NULL, and so may each
 * entry.  The parameter gradients are sums over per-workgroup partials in a fixed order (bit-identical from run to run).
 * ws: recnow_attention_dnn_workspace_bytes(..., backward) bytes for that direction, bounded independently of B and L
 * (0 when B or L is 0).  D > 256, a width > 256 or nl > 4: RECNOW_EUNSUPPORTED. */
size_t recnow_attention_dnn_workspace_bytes(int64_t B, int L, int D, int nl, const int* dims_host, int backward);
int recnow_attention_dnn_fwd(const float* user, const float* doc, int64_t B, int L, int D, int nl, const int* dims_host,
                             const float* const* kernels_host, const float* const* biases_host, int act, float* mat,
                             float* score_sum, void* ws, size_t ws_bytes, void* stream);
int recnow_attention_dnn_bwd(const float* user, const float* doc, int64_t B, int L, int D, int nl, const int* dims_host,
                             const float* const* kernels_host, const float* const* biases_host, int act, const float* dmat,
                             const float* dsum, float* duser, float* ddoc, float* const* dkernels_host,
                             float* const* dbiases_host, void* ws, size_t ws_bytes, void* stream);

/* focal_crossentropy_loss: rec_now/rec_block/focal_loss.py:12-66.  alpha <= 0 / gamma <= 0 switch the respective factor
 * off (the reference's `if alpha:` / `if gamma:`).  loss_elem (B) and/or loss_mean (1) may be NULL; the mean is summed in
 * double in a fixed order (ws: recnow_focal_loss_workspace_bytes).
 * Backward: dlogits[i] = dloss_i/dlogit_i * (gelem ? gelem[i] : 1) * (gscalar ? *gscalar : 1) * scale  (scale = 1/B for the
 * mean); stop_weight_gradient as :60-61. */
size_t recnow_focal_loss_workspace_bytes(int64_t B);
int recnow_focal_loss_fwd(const float* labels, const float* logits, int64_t B, float alpha, float gamma, float* loss_elem,
                          float* loss_mean, void* ws, size_t ws_bytes, void* stream);
int recnow_focal_loss_bwd(const float* labels, const float* logits, int64_t B, float alpha, float gamma,
                          int stop_weight_gradient, const float* gelem, const float* gscalar, float scale, float* dlogits,
                          void* stream);

/* Pooled embedding lookup by slot: rec_now/rec_block/embedding_util.py:239-324 (and :138-195 for the slot -> target map).
 *   recnow_slot_targets:   seg[i] = index of slots[i] in targets[0..T) or -1;  key[i] (optional) = ids[i] if seg[i] >= 0 else
 *                          INT64_MIN (sorts after every id >= 0 as an unsigned radix key in recnow_group_segments, and costs
 *                          one extra 8-bit pass where all-ones cost five).  slot_dtype: RECNOW_KEY_I32/I64
 *                          (slots and targets share it; targets is a DEVICE array).  N = B*C entries.
 *   recnow_embed_pool_fwd: out[b][t][:] = sum_{c: seg[b][c]==t} weights[b][c] * table[rows[b][c]][:]  (mean != 0: divided by the
 *                          number of pooled entries, empty segments 0 - tf.math.unsorted_segment_mean).  rows: row index into
 *                          `table` per entry (the ids themselves, or the inverse index of recnow_embed_unique); weights, cnt
 *                          (B,T entry counts, needed by the 'mean' backward) may be NULL.  No atomics: fixed summation order.
 *                          V = rows of `table`: an entry whose row index is outside [0, V) adds a zero row (it still counts
 *                          for 'mean'), the same entries recnow_embed_scatter_rows drops in the backward.
 *   recnow_embed_pool_bwd_weights: dweights[b][c] = <dout[b][seg[b][c]], table[rows[b][c]]> (/ cnt for 'mean'), 0 for entries
 *                          that are not pooled or whose row is outside the table: the gradient TF autodiff gives `weights`.
 *   recnow_embed_unique:   from the sort of `key` (recnow_group_keys(I64) + recnow_group_segments): unique[s] = id of sorted
 *                          segment s, inverse[entry] = s, *n_unique = number of real ids (the INT64_MIN segment excluded).
 *   recnow_embed_rows_bwd: drows[s][:] = sum over the entries of segment s of w * dout[b][t][:] (/cnt): the gradient of row
 *                          unique[s]; row_ids[s] = that id (INT64_MIN for the unpooled segment and for unused slots s >= n_seg).
 *                          drows / row_ids hold N slots.  The entry range is cut into fixed chunks (a hot id may own millions of
 *                          entries); pieces are joined in ascending chunk order (ws: recnow_embed_rows_bwd_workspace_bytes).
 *   recnow_embed_scatter_rows: dtable[row_ids[s]][:] = drows[s][:] into a zero-initialised dense (V,D) gradient. */
/* id_limit / key32 (ABI 4): id_limit = V > 0 says the ids index a table of V rows (V < 2^31 - 1): entries that are not pooled AND ids outside
 * [0, V) then carry the key V instead of INT64_MIN -- it sorts last and is dropped like every id outside the table -- and key32 (optional,
 * N int32) receives the same keys as 32-bit values: the sort of the backward pass runs on ONE key word (three 8-bit digit passes for
 * V = 2^20 instead of four on two words).  id_limit = 0, key32 = NULL: the INT64_MIN form (ids of unknown range: the unique path). */
int recnow_slot_targets(const void* slots, int slot_dtype, const void* targets, int T, const int64_t* ids, int64_t N,
                        int32_t* seg, int64_t* key, int64_t id_limit, int32_t* key32, void* stream);
int recnow_embed_pool_fwd(const float* table, int D, int64_t V, const int64_t* rows, const int32_t* seg, const float* weights,
                          int64_t B, int C, int T, int mean, float* out, float* cnt, void* stream);
int recnow_embed_pool_bwd_weights(const float* table, int D, int64_t V, const int64_t* rows, const int32_t* seg, const float* cnt,
                                  const float* dout, int64_t B, int C, int T, int mean, float* dweights, void* stream);
int recnow_embed_unique(const int64_t* key, const int32_t* order, const int32_t* seg_id, const int32_t* seg_first,
                        const int32_t* n_seg, int64_t N, int64_t* unique, int64_t* inverse, int32_t* n_unique, void* stream);
size_t recnow_embed_rows_bwd_workspace_bytes(int64_t N, int D);
int recnow_embed_rows_bwd(const int64_t* key, const int32_t* order, const int32_t* seg_id, const int32_t* seg_first,
                          const int32_t* n_seg, const int32_t* seg, const float* weights, const float* cnt, const float* dout,
                          int64_t N, int C, int T, int D, int mean, float* drows, int64_t* row_ids, void* ws, size_t ws_bytes,
                          void* stream);
/* n_seg (ABI 4, optional DEVICE pointer: the segment count of recnow_group_segments): only the first n_seg[0] slots are read. */
int recnow_embed_scatter_rows(const float* drows, const int64_t* row_ids, int64_t n_slots, int D, int64_t V, float* dtable,
                              const int32_t* n_seg, void* stream);
/* (ABI 10) recnow_embed_rows_bwd for lookups whose every key is a row of ONE dense (V, D) gradient: dtable (zero-filled by the caller)
 * receives dtable[key][:] = sum over the entries e with that key of w * dout[e / C][:], w = weights[e / w_div] (weights NULL: 1), straight from
 * the sorted segments -- no slot buffer of N rows, no scatter pass.  A key outside [0, V) is dropped.  Same fixed summation order, same ws. */
int recnow_embed_rows_bwd_direct(const int64_t* key, const int32_t* order, const int32_t* seg_id, const int32_t* seg_first,
                                 const int32_t* n_seg, const float* weights, int w_div, const float* dout, int64_t N, int C, int D,
                                 float* dtable, int64_t V, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Single-slot fetch, sequence embedding and slot pooling (ABI 11): rec_now/rec_block/embedding_util.py:531-584 (fetch_single_slot),
 * :327-416 (embedding_single_slot), :419-489 (pool_slots).  slots / ids / weights are (B, C); slot_dtype, id_dtype, row_dtype are
 * RECNOW_KEY_I32 / RECNOW_KEY_I64; `target` is compared as a 64-bit value.  One wave per batch row, selection by 64-bit ballot; every element
 * of every output is written by the kernel (outputs may be uninitialised), nothing is allocated, no atomics on float data.
 *   recnow_slot_max_count: *max_count (DEVICE int32) = max over the rows of the number of entries whose slot is `target` (what ncols=None means).
 *   recnow_slot_fetch:     row b of each output (B, ncols) = the entries of row b whose slot is `target`, in column order, cut to the first ncols
 *                          or filled up: out_ids (dtype of ids) with default_id, out_weights with default_weight, mask (bytes) 1 / 0, src (int32)
 *                          the source column / -1.  Each output (and its input) may be NULL.
 *   recnow_slot_fetch_bwd: dweights[b][c] = dout[b][j] where src[b][j] == c, 0 elsewhere (dweights (B, C), dout (B, ncols)).
 *   recnow_slot_embed_fwd: the same selection fused with the gather: out[b][j][:] = table[rows[b][c_j]][:] (out (B, ncols, D)), a zero row for
 *                          filled-up positions and for row indices outside [0, V).  rows: per entry the row of `table` -- the ids themselves, or
 *                          the inverse index of recnow_embed_unique -- as int32 or int64.  16-byte copies when D % 4 == 0 and table and out are
 *                          16-byte aligned, element-wise otherwise (any D >= 1).  out_weights / mask / src as recnow_slot_fetch.  key / key32
 *                          (optional, (B, ncols)): per output position the table row, or for filled-up positions and rows outside the table
 *                          key_limit (= V > 0; key32 needs V < 2^31 - 1) or INT64_MIN (key_limit = 0) -- the convention of recnow_slot_targets.
 *                          The table gradient is recnow_embed_rows_bwd_direct (or recnow_embed_rows_bwd) over the B * ncols positions with
 *                          these keys, C = 1, dout one row per position: fixed summation order, bit-identical from run to run.
 *   recnow_slot_pool_fwd:  seg (B, C) from recnow_slot_targets (T targets).  out_ids[b][t] = min of ids over the kept entries of segment t, 0 if
 *                          there is none or the minimum is the dtype's maximum; out_weights[b][t] = their sum of weights (mean != 0: divided by
 *                          their number, empty 0); cnt[b][t] (optional) = that number.  drop_duplicate != 0: an entry is not kept when the column
 *                          immediately before it has the same seg.  Sums add in ascending column order.  ids / weights pairs may be NULL.
 *   recnow_slot_pool_bwd:  dweights[b][c] = dout[b][seg[b][c]] (/ cnt for mean) for kept entries, 0 otherwise.
 * ---------------------------------------------------------------------------------------------------------- */
int recnow_slot_max_count(const void* slots, int slot_dtype, int64_t target, int64_t B, int C, int32_t* max_count, void* stream);
int recnow_slot_fetch(const void* slots, int slot_dtype, int64_t target, const void* ids, int id_dtype, const float* weights,
                      int64_t B, int C, int ncols, int64_t default_id, float default_weight, void* out_ids, float* out_weights,
                      uint8_t* mask, int32_t* src, void* stream);
int recnow_slot_fetch_bwd(const int32_t* src, const float* dout, int64_t B, int C, int ncols, float* dweights, void* stream);
int recnow_slot_embed_fwd(const float* table, int D, int64_t V, const void* slots, int slot_dtype, int64_t target, const void* rows,
                          int row_dtype, const float* weights, int64_t B, int C, int ncols, float default_weight, float* out,
                          float* out_weights, uint8_t* mask, int32_t* src, int64_t* key, int32_t* key32, int64_t key_limit, void* stream);
int recnow_slot_pool_fwd(const int32_t* seg, const void* ids, int id_dtype, const float* weights, int64_t B, int C, int T, int mean,
                         int drop_duplicate, void* out_ids, float* out_weights, float* cnt, void* stream);
int recnow_slot_pool_bwd(const int32_t* seg, const float* cnt, const float* dout, int64_t B, int C, int T, int mean, int drop_duplicate,
                         float* dweights, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * MultiHashLayer / FastMultiHashLayer (ABI 10): rec_now/layers/multi_hash_layer.py.  bucket_h(id) = hash_h(text of id) % num_bins (unsigned
 * 64-bit), hash_h = SipHash-2-4 keyed (salts[h], salts[h]) -- keras Hashing(salt=(s, s)) -- or, for h = 0 with first_unsalted, FarmHash
 * Fingerprint64 -- Hashing(salt=None).  The text of an integer id is its "%lld" decimal form.  salts: HOST array of num_hash values >= 0;
 * 1 <= num_hash <= 16; num_bins >= 1; id_dtype RECNOW_KEY_I32 / RECNOW_KEY_I64.  Buckets are int64, out[i * num_hash + h].
 *   recnow_hash_ids_host / recnow_hash_bytes_host: on the HOST, no GPU call (host pointers throughout).  bytes_host: string i is
 *     bytes[offsets[i] .. offsets[i + 1]); with first_unsalted a string longer than 32 bytes returns RECNOW_EUNSUPPORTED (Fingerprint64 is
 *     implemented for 0..32 bytes), never a wrong bucket.  SipHash takes any length.
 *   recnow_hash_ids: the same on the device (ids, out DEVICE).
 *   recnow_hash_embed_fwd: ids (B, L) -> hash, gather and reduce in one pass.  tables_host: HOST array of num_hash DEVICE pointers to (num_bins, D)
 *     fp32 row blocks (one table per hash function, or slices h * num_bins of one table).  id_dtype RECNOW_HASH_BUCKETS: `ids` holds (B, L, num_hash)
 *     int64 bucket numbers computed elsewhere (recnow_hash_bytes_host); a bucket outside [0, num_bins) reads as a zero row.  mode:
 *       RECNOW_HASH_SUM / _MEAN  out (B, L, D)            sum (mean) over the hash functions
 *       RECNOW_HASH_ROWS         out (B, L, num_hash, D)  the rows themselves (bit-identical copies)
 *       RECNOW_HASH_POOLED       out (B, D) = sum_l weights[b][l] * sum_h row; weights (B, L) or NULL (other modes: must be NULL)
 *     keys (B, L, num_hash) int64 / keys32 the same as int32, both optional: h * num_bins + bucket, the sort key of the table gradient
 *     (recnow_embed_rows_bwd_direct over a (num_hash * num_bins, D) buffer) and what recnow_hash_embed_bwd_weights gathers from.
 *     Fixed summation order, no atomics.  16-byte gathers when D % 4 == 0 and tables and out are 16-byte aligned, else element-wise (any D >= 1).
 *     num_hash * num_bins or B * L * num_hash >= 2^31, or pooled with more than 256 gather elements per row (D > 1024, or D > 256 unaligned):
 *     RECNOW_EUNSUPPORTED.
 *   recnow_hash_embed_bwd_weights: dweights[b][l] = <dout[b][:], sum_h row> for the pooled mode, rows re-gathered from `keys`.
 * ---------------------------------------------------------------------------------------------------------- */
#define RECNOW_HASH_BUCKETS 4
#define RECNOW_HASH_SUM 0
#define RECNOW_HASH_MEAN 1
#define RECNOW_HASH_ROWS 2
#define RECNOW_HASH_POOLED 3
int recnow_hash_ids_host(const void* ids, int id_dtype, int64_t n, const int64_t* salts, int num_hash, int first_unsalted,
                         int64_t num_bins, int64_t* out);
int recnow_hash_bytes_host(const unsigned char* bytes, const int64_t* offsets, int64_t n, const int64_t* salts, int num_hash,
                           int first_unsalted, int64_t num_bins, int64_t* out);
int recnow_hash_ids(const void* ids, int id_dtype, int64_t n, const int64_t* salts_host, int num_hash, int first_unsalted,
                    int64_t num_bins, int64_t* out, void* stream);
int recnow_hash_embed_fwd(const void* ids, int id_dtype, int64_t B, int64_t L, const int64_t* salts_host, int num_hash,
                          int first_unsalted, int64_t num_bins, const float* const* tables_host, int D, const float* weights,
                          int mode, float* out, int64_t* keys, int32_t* keys32, void* stream);
int recnow_hash_embed_bwd_weights(const int64_t* keys, const float* const* tables_host, int num_hash, int64_t num_bins, int D,
                                  const float* dout, int64_t B, int64_t L, float* dweights, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * CartesianProductLayer (ABI 14): rec_now/layers/cartesian_product_layer.py feeding MultiHashLayer / FastMultiHashLayer.  Element (b, j) of the
 * (B, P) cross, P = len[0] * ... * len[n_inputs - 1], j row-major with the LAST input fastest, is the text
 *     str(ids[0][b][j0]) SEP str(ids[1][b][j1]) SEP ...          (decimal "%lld" texts; input k is (B, len[k]), or (1, len[k]) with batch1[k])
 * which is never stored: the kernels compose it per element and hash it like the text of a plain id.  Invalid patterns: input i may carry up to 8
 * literal alternatives (n_alt[i] = 0: no pattern; a literal may be empty).  The element is replaced by the default string when the regular
 * expression ^.*SEP ... (lit_a|lit_b|...) ... SEP.*$ -- the group in position i -- matches the JOINED text, which is decided exactly (csrc/hash64.hpp,
 * rn_cross_match); its buckets are then default_buckets[h], computed by the caller (recnow_hash_bytes_host) and required to lie in [0, num_bins).
 * Words are little-endian: byte p of a text is bits 8 (p % 8) of word p / 8, zero padded.
 * Limits (RECNOW_EINVAL beyond them): 1..4 inputs, separator <= 4 bytes, worst-case text (11 bytes per int32 input, 20 per int64 input, plus the
 * separators) <= 96 bytes, default string <= 96 bytes, literals <= 24 bytes.  With first_unsalted (Fingerprint64, 0..32 bytes) a worst-case text or
 * a default string longer than 32 bytes is RECNOW_EUNSUPPORTED; B * P * num_hash >= 2^31 as well.
 *   recnow_cross_text / _host: text (B, P, W) uint8 zero padded, W a multiple of 8 and >= the worst-case text and the default string; lens (B, P) int32.
 *   recnow_cross_hash_ids / _host: (B * P, num_hash) int64 bucket numbers.
 *   recnow_cross_hash_embed_fwd: recnow_hash_embed_fwd with L = P and the ids taken from the descriptor; keys / keys32 as there, so the backward
 *     entry points serve unchanged.
 * The *_host twins run the same code on the host (host pointers in the descriptor, no GPU call).  No allocation, no host synchronisation.
 * ---------------------------------------------------------------------------------------------------------- */
#define RECNOW_CROSS_MAX_INPUTS 4
#define RECNOW_CROSS_MAX_SEP 4
#define RECNOW_CROSS_MAX_TEXT 96
#define RECNOW_CROSS_MAX_ALTS 8
#define RECNOW_CROSS_MAX_LIT 24
typedef struct recnow_cross_desc {
    const void* ids[RECNOW_CROSS_MAX_INPUTS];        /* (B, len[k]) or (1, len[k]) contiguous ids */
    int32_t dtype[RECNOW_CROSS_MAX_INPUTS];          /* RECNOW_KEY_I32 / RECNOW_KEY_I64 */
    int32_t len[RECNOW_CROSS_MAX_INPUTS];
    int32_t batch1[RECNOW_CROSS_MAX_INPUTS];         /* 1: one row shared by the whole batch */
    int32_t n_inputs;
    int32_t sep_len;
    uint32_t sep_word;                               /* the separator's bytes */
    int32_t default_len;
    int32_t n_alt[RECNOW_CROSS_MAX_INPUTS];
    int32_t lit_len[RECNOW_CROSS_MAX_INPUTS][RECNOW_CROSS_MAX_ALTS];
    uint64_t lit_words[RECNOW_CROSS_MAX_INPUTS][RECNOW_CROSS_MAX_ALTS][RECNOW_CROSS_MAX_LIT / 8];
    uint64_t default_words[RECNOW_CROSS_MAX_TEXT / 8]; /* the default string's bytes (recnow_cross_text) */
    int64_t default_buckets[16];                     /* its bucket under each hash function (the hash entry points) */
} recnow_cross_desc;
int recnow_cross_text_host(recnow_cross_desc desc, int64_t B, int W, unsigned char* text, int32_t* lens);
int recnow_cross_hash_ids_host(recnow_cross_desc desc, int64_t B, const int64_t* salts, int num_hash, int first_unsalted, int64_t num_bins,
                               int64_t* out);
int recnow_cross_text(recnow_cross_desc desc, int64_t B, int W, unsigned char* text, int32_t* lens, void* stream);
int recnow_cross_hash_ids(recnow_cross_desc desc, int64_t B, const int64_t* salts_host, int num_hash, int first_unsalted, int64_t num_bins,
                          int64_t* out, void* stream);
int recnow_cross_hash_embed_fwd(recnow_cross_desc desc, int64_t B, const int64_t* salts_host, int num_hash, int first_unsalted,
                                int64_t num_bins, const float* const* tables_host, int D, const float* weights, int mode, float* out,
                                int64_t* keys, int32_t* keys32, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * StarDenseLayer / StackedDenseLayer (ABI 7): rec_now/layers/star_dense_layer.py:118-163, stacked_dense_layer.py:116-155.
 * A Dense layer personalised per row by K <= 4 parameter rows.  params_host / dparams_host: HOST arrays of K DEVICE pointers to
 * contiguous (B, R) fp32 tensors, R = D*U + U: the first D*U entries of a row are a kernel [d][u], the last U a bias.
 *   RECNOW_STAR_MUL: Weff[b] = kernel * prod_k P_k[b][:DU]           beff[b] = sum_k P_k[b][DU:] + bias - K
 *   RECNOW_STAR_ADD: Weff[b] = kernel + weight * sum_k P_k[b][:DU]   beff[b] = bias + weight * sum_k P_k[b][DU:]
 *   y[b] = act(x[b] . Weff[b] + beff[b]);  x (B,D), kernel (D,U), bias (U) or NULL, y (B,U).
 * No (B,D,U) tensor is formed: each P_k element is read once.  Backward, from y (act' through the output) and dy:
 *   dx (may be NULL); dparams_host (may be NULL, and so may each entry: that dP_k is not written); dkernel, dbias (may be NULL).
 *   dkernel / dbias are sums over fixed batch chunks in a fixed order (ws: recnow_star_dense_workspace_bytes, needed only
 *   when one of them is requested; it is bounded by the backward's workgroups x R floats, independent of B).
 *   K > 4: RECNOW_EUNSUPPORTED.
 * ---------------------------------------------------------------------------------------------------------- */
#define RECNOW_STAR_MUL 0
#define RECNOW_STAR_ADD 1
size_t recnow_star_dense_workspace_bytes(int64_t B, int D, int U);
int recnow_star_dense_fwd(const float* x, const float* const* params_host, int K, int mode, float weight, const float* kernel,
                          const float* bias, int64_t B, int D, int U, int act, float* y, void* stream);
int recnow_star_dense_bwd(const float* x, const float* const* params_host, int K, int mode, float weight, const float* kernel,
                          const float* y, const float* dy, int64_t B, int D, int U, int act, float* dx, float* const* dparams_host,
                          float* dkernel, float* dbias, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * SparseGNNLayer (ABI 9): rec_now/layers/sparse_gnn_layer.py:227-236.  L layers  v <- act(v + W_l^T v)  on the F-vector v of every
 * (row, channel) pair, W_l[src_e][dst_e] = w[l % n_sets][e] for the E edges e.  One launch per direction runs all L layers on tiles that
 * stay in LDS: the forward reads x once and writes every requested layer output once; the backward reads x and the output gradients,
 * RECOMPUTES the layer chain of its tile, and writes dx (it needs no saved activation).  F <= 64 and E <= 4096: else RECNOW_EUNSUPPORTED.
 *   layouts: RECNOW_GNN_BFD x (B,F,D) contiguous (also (B,F*D)); RECNOW_GNN_BDF x (B,D,F) contiguous; RECNOW_GNN_LIST x_fields = DEVICE
 *     array of F pointers to contiguous (B,D) tensors (x_aligned: every one of them is 16-byte aligned).  Outputs and their gradients
 *     are BFD or BDF (out_layout).  dx has the layout of the input; for RECNOW_GNN_LIST it is one (F,B,D) block.
 *   tab: DEVICE int32 array  Cd | Cs | 0 | 0 | dS (Cd x 8) | dG (Cd x 4) | sS (Cs x 8) | sG (Cs x 4) | ssrc (E) | sdst (E) | swid (E).
 *     A pass over the graph walks a stream of CHUNKS of four edges of one node, in node order (a node without edges has one chunk; a short
 *     chunk is padded with edges of weight index -1 that point at the node itself).  S: o0 o1 o2 o3 node flags 0 0 (flags: 1 first chunk of
 *     the node | 2 last); G: the four weight indices.  dS / dG: by destination, o = the sources of the edges into `node` (Cd chunks, the
 *     forward); sS / sG: by source, o = the destinations of the edges out of `node` (Cs chunks, the input gradient); ssrc / sdst / swid:
 *     source, destination and weight index of every edge (the weight gradient).  Every index must be < F (fields) or < E (weights).
 *   w (n_sets, E).  act: enum recnow_act.  y_last or NULL; y_all: NULL or a DEVICE array of L pointers, entry l (may be 0) receives
 *     layer l's output (y_aligned: all 16-byte aligned).  dy_last / dy_all / dy_aligned likewise: every gradient given is added in.
 *   dx, dw (n_sets, E) may be NULL.  dw is a fixed-order sum (no float atomics): ws of recnow_sparse_gnn_workspace_bytes, needed only
 *     with dw; it is bounded by the backward's workgroups (<= 1024) x n_sets x E floats, independent of B.
 * ---------------------------------------------------------------------------------------------------------- */
#define RECNOW_GNN_BFD 0
#define RECNOW_GNN_BDF 1
#define RECNOW_GNN_LIST 2
size_t recnow_sparse_gnn_workspace_bytes(int64_t B, int F, int D, int E, int n_sets);
int recnow_sparse_gnn_fwd(const float* x, const float* const* x_fields, int in_layout, int x_aligned, int out_layout, const int32_t* tab,
                          const float* w, int64_t B, int F, int D, int E, int L, int n_sets, int act, float* y_last, float* const* y_all,
                          int y_aligned, void* stream);
int recnow_sparse_gnn_bwd(const float* x, const float* const* x_fields, int in_layout, int x_aligned, int out_layout, const int32_t* tab,
                          const float* w, int64_t B, int F, int D, int E, int L, int n_sets, int act, const float* dy_last,
                          const float* const* dy_all, int dy_aligned, float* dx, float* dw, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * SparseGNNLayer, the dense route (ABI 15): the same layer with the graph as a dense matrix on the matrix cores (csrc/sparse_gnn_dense.hip),
 * for F <= 128 and E <= F * F: else RECNOW_EUNSUPPORTED.  Per call a small launch scatters w into M = I + W (n_sets, 2, FP, FP), FP = F rounded
 * up to 32, plane 1 the transpose; a layer over a tile of (row, channel) pairs is then one exact-fp32 product on v_mfma_f32_32x32x2_f32
 * whatever the number of edges.  One launch per direction runs all L layers on tiles in LDS; the backward recomputes the chain and forms
 * dM = sum over pairs of v_in dz^T as a product over the pairs, added to one workspace row per workgroup; a second launch sums the rows in
 * row order at the edge positions into dw (no float atomics: dx and dw are bit-identical from run to run).
 *   Arguments as recnow_sparse_gnn_fwd / _bwd, except: src, dst: DEVICE int32 arrays of E entries, the edges [source, destination] in
 *     ascending order (entry e belongs to w[.][e]; every index < F; no edge twice) instead of `tab`; ws of
 *     recnow_sparse_gnn_dense_workspace_bytes(F, E, n_sets, backward): the dense matrices, and with backward != 0 (needed only with dw) the
 *     rows of dM: at most 1024 rows and at most 32 MB (but 16 rows), independent of B and D.  16-byte aligned.  Both directions need it.
 * ---------------------------------------------------------------------------------------------------------- */
size_t recnow_sparse_gnn_dense_workspace_bytes(int F, int E, int n_sets, int backward);
int recnow_sparse_gnn_dense_fwd(const float* x, const float* const* x_fields, int in_layout, int x_aligned, int out_layout, const int32_t* src,
                                const int32_t* dst, const float* w, int64_t B, int F, int D, int E, int L, int n_sets, int act, float* y_last,
                                float* const* y_all, int y_aligned, void* ws, size_t ws_bytes, void* stream);
int recnow_sparse_gnn_dense_bwd(const float* x, const float* const* x_fields, int in_layout, int x_aligned, int out_layout, const int32_t* src,
                                const int32_t* dst, const float* w, int64_t B, int F, int D, int E, int L, int n_sets, int act,
                                const float* dy_last, const float* const* dy_all, int dy_aligned, float* dx, float* dw, void* ws,
                                size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Tensor plumbing (ABI 12): rec_now/layers/pooling_layer.py (PoolingLayer), rec_now/layers/fix_length_layer.py (pad_or_truncate,
 * FixLengthLayer), rec_now/rec_block/embedding_wise_weight.py (gather_embedding_element_wise_weight).  csrc/tensor_util.hip.
 * Every contiguous tensor is given as (O, R, I): outer extent, the axis worked on, inner extent.  fp32 unless said otherwise.
 * An empty extent (O, I, P or B equal to 0) returns RECNOW_OK without a launch.  No float atomics: bit-identical from run to run.
 *   recnow_reduce_axis_fwd: out (O, I) = sum / mean / max / min of x (O, R, I) over R; R >= 1.  ws of
 *     recnow_reduce_axis_workspace_bytes (0 except for one long row, O == 1 and I == 1: the partials of the two-stage reduction).
 *   recnow_reduce_axis_bwd: dx (O, R, I) from g (O, I).  sum: g; mean: g * (1 / R); max / min: TensorFlow's rule, g / count at every
 *     position equal to the result y (O, I), count = the number of such positions of the run (x and y are read only for max / min).
 *   recnow_pad_axis: out (O, L_out, I) = x cut to, or filled up with the element `fill_bits` to, L_out along the middle axis; elements of
 *     elt_bytes = 4 or 8 bytes, copied as bits (fill_bits: the element's bit pattern in the low bytes).  Its own backward: the gradient
 *     of (O, L_out, I) padded or cut back to L_in with fill 0.
 *   recnow_elem_weight_fwd: out[b][p] = w[b][pos[p]], times x[b][p] when x is given; w (B, E), pos (P) int32 DEVICE entries in [0, E)
 *     (the caller checks them; the kernel does not), x and out (B, P).  P <= 2^24.
 *   recnow_elem_weight_bwd: dw[b][e] = sum over {p : pos[p] == e}, in ascending p, of g[b][p] (* x[b][p] when x is given) through the
 *     inverse of pos as a CSR table: off (E + 1) and idx (P) int32 DEVICE arrays, idx[off[e] .. off[e + 1]) = the positions of e.
 *     dx[b][p] = g[b][p] * w[b][pos[p]] in the same launch.  dw, dx may each be NULL (w, pos are read only for dx).
 * ---------------------------------------------------------------------------------------------------------- */
#define RECNOW_REDUCE_SUM 0
#define RECNOW_REDUCE_MEAN 1
#define RECNOW_REDUCE_MAX 2
#define RECNOW_REDUCE_MIN 3
size_t recnow_reduce_axis_workspace_bytes(int64_t O, int64_t R, int64_t I);
int recnow_reduce_axis_fwd(const float* x, int64_t O, int64_t R, int64_t I, int op, float* out, void* ws, size_t ws_bytes, void* stream);
int recnow_reduce_axis_bwd(const float* x, const float* y, const float* g, int64_t O, int64_t R, int64_t I, int op, float* dx,
                           void* stream);
int recnow_pad_axis(const void* x, int elt_bytes, int64_t O, int64_t L_in, int64_t L_out, int64_t I, int64_t fill_bits, void* out,
                    void* stream);
int recnow_elem_weight_fwd(const float* w, const int32_t* pos, const float* x, int64_t B, int E, int P, float* out, void* stream);
int recnow_elem_weight_bwd(const float* g, const float* x, const float* w, const int32_t* pos, const int32_t* off, const int32_t* idx,
                           int64_t B, int E, int P, float* dw, float* dx, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * CANLayer, the co-action network (ABI 13): rec_now/layers/can_layer.py:228-275.  csrc/can.hip.
 * Every sample b carries its own small MLP in params (B, P): layer after layer, a kernel (D_{k-1}, D_k) row-major, then (use_bias) a
 * bias (D_k); P = sum_k D_{k-1} D_k [+ D_k].  dims: HOST array of the n_layers output widths D_1 .. D_n.  x (B, L, D0):
 *   h_0 = x[b][l];  o = h_{k-1} . W_k[b] (+ bias_k[b]);  a = act(o) on every layer but the last (on the last too with last_act);
 *   h_k = a (+ h_{k-1} with res_net: then every width must equal D0, else RECNOW_EINVAL);
 *   out[b][l] = h_n * any(x[b][l][:] != 0) with mask (else h_n).
 * combiner -1: y (B, L, D_n) = out.  combiner RECNOW_REDUCE_*: y (B, D_n) = sum / mean / max / min of out over l (masked positions
 * count as zeros); L >= 1 then (else RECNOW_EINVAL).  One launch per direction, one workgroup per sample, the sample's parameters in
 * LDS; no (B, L, D) intermediate, no workspace, no float atomics: the same input gives the same bits on every run.
 * recnow_can_bwd recomputes the layer chain (it reads no saved activation) from x, params, g (the gradient of y) and, for max / min
 * only, y: every position whose output equals y shares g / count.  dx (B, L, D0) and dparams (B, P) may each be NULL; every element
 * of the ones given is written once.
 * recnow_can_supported: host-only (no device call), 1 exactly for the shapes the kernels take: D0 and every width in 1..64,
 * 1..8 layers, and P floats plus the backward's staging within the 64 KB of LDS one workgroup asks for.  Other shapes:
 * RECNOW_EUNSUPPORTED from _fwd / _bwd.  B == 0 returns RECNOW_OK without a launch.
 * ---------------------------------------------------------------------------------------------------------- */
int recnow_can_supported(int D0, const int* dims, int n_layers, int use_bias);
int recnow_can_fwd(const float* x, const float* params, float* y, int64_t B, int64_t L, int D0, const int* dims, int n_layers, int act,
                   int use_bias, int res_net, int last_act, int mask, int combiner, void* stream);
int recnow_can_bwd(const float* x, const float* params, const float* g, const float* y, int64_t B, int64_t L, int D0, const int* dims,
                   int n_layers, int act, int use_bias, int res_net, int last_act, int mask, int combiner, float* dx, float* dparams,
                   void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * BilinearInteractionLayer (ABI 25): the bilinear cross of FiBiNET (Huang, Zhang and Zhang 2019, arXiv 1905.09433, section 3.3).
 * csrc/bilinear.hip.  fields / dfields: DEVICE arrays of F device pointers to contiguous (B, D) fp32 tensors, as for InnerPNN; the
 * P = F(F-1)/2 pairs (i, j), i < j, in InnerPNN's i-major order, pair p at i*F - i(i+1)/2 + (j - i - 1).
 *   out[b][p*D + d] = (x_i[b] W[w(p)])[d] * x_j[b][d],   out (B, P*D),   W (nW, D, D) row-major
 *   type RECNOW_BILINEAR_ALL: w(p) = 0, nW = 1;  _EACH: w(p) = i, nW = F-1;  _INTERACTION: w(p) = p, nW = P.
 * fp32 FMA on exact fp32 operands; U = X W is formed on chip and never written.  F == 1 or B == 0: RECNOW_OK without a launch
 * from _fwd.  recnow_bilinear_bwd recomputes U and writes every row of every dfields[f] once (zeros for F == 1); with dW non-NULL
 * it also writes the weight gradient (nW, D, D): fp32 sums per row chunk, the chunks combined in fp64 in a fixed order -- no
 * float atomics, the same input gives the same bits on every run.  ws is only needed with dW: recnow_bilinear_workspace_bytes =
 *   ['all', 'each': 4 B (F-1) D, the dU rows] + 4 G S D^2 (S = F-1 or P slots, G <= 256 row chunks, G S D^2 floats <= 32 MiB or
 *   G = 1), each part rounded up to 256 bytes; it does not grow as B P D^2.
 * recnow_bilinear_supported: host-only, 1 for 1 <= F <= 64, 1 <= D <= 64 and a known type; other shapes: RECNOW_EUNSUPPORTED from
 * _fwd / _bwd.  16-byte accesses need D % 4 == 0 and 16-byte aligned tensors; anything else takes guarded 4-byte accesses in the
 * same kernels.  recnow_bilinear_route: host-only, the kernel family of a direction (bwd 0 / 1): 0 one wave per sample with the
 * weights resident in LDS, 1 the same with the weights read through L2 (they do not fit), 2 a tile of samples per workgroup with
 * the weights of a batch of pairs staged per tile ('interaction').
 * ---------------------------------------------------------------------------------------------------------- */
#define RECNOW_BILINEAR_ALL 0
#define RECNOW_BILINEAR_EACH 1
#define RECNOW_BILINEAR_INTERACTION 2
int recnow_bilinear_supported(int F, int D, int type);
int recnow_bilinear_route(int F, int D, int type, int bwd);
size_t recnow_bilinear_workspace_bytes(int64_t B, int F, int D, int type);
int recnow_bilinear_fwd(const float* const* fields, int F, int64_t B, int D, int type, const float* W, float* out, void* stream);
int recnow_bilinear_bwd(const float* const* fields, float* const* dfields, int F, int64_t B, int D, int type, const float* W,
                        const float* dout, float* dW, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * InteractingLayer (ABI 26): the multi-head self-attention over the fields of AutoInt (Song et al. 2019, arXiv 1810.11921,
 * section 4.3).  csrc/autoint.hip.  fields / dfields: DEVICE arrays of F device pointers; field f of sample b is the D floats at
 * fields[f] + b * xstride (dfields[f] + b * dxstride), one row stride in floats for all fields, >= D -- a (B, F, D) tensor and the
 * column views of a (B, F*D) tensor pass without a copy.  H heads of width d, E = H d; Wq, Wk, Wv, Wr (D, E) row-major, Wr NULL
 * without the residual projection.
 *   Q = X Wq, K = X Wk, V = X Wv;  S_h = Q_h K_h^T (times 1/sqrt(d) with scaling != 0);  A_h = softmax over the keys, row maximum
 *   subtracted;  pre = concat_h A_h V_h (+ X Wr);  out[b][f*E + e] = relu(pre) (relu != 0) or pre,  out (B, F*E) contiguous.
 * fp32 FMA on exact fp32 operands, the exponential through the hardware exp2; Q, K, V, S, A and pre stay on chip.  B == 0:
 * RECNOW_OK without a launch.  recnow_autoint_bwd recomputes the chain from the fields and writes every row of every dfields[f]
 * once; the ReLU subgradient at 0 is 0.  dWq, dWk, dWv (and dWr with Wr) are either all given or all NULL; NULL: no weight-gradient
 * launch and ws is not read.  Otherwise fp32 partials per workgroup (a contiguous chunk of samples) are combined in fp64 in a
 * fixed tree: no float atomics, the same input gives the same bits on every run.  recnow_autoint_workspace_bytes =
 *   4 G nW D E rounded up to 256 bytes, nW = 3 + use_res, G = max(1, min(ceil(B / 8), 1024, 32 MiB / (4 nW D E))).
 * recnow_autoint_supported: host-only, 1 for 1 <= F, D, E <= 64 and 1 <= H <= 8; other shapes: RECNOW_EUNSUPPORTED from _fwd /
 * _bwd.  16-byte accesses need widths and row strides that are multiples of 4 floats and 16-byte aligned bases; anything else
 * takes guarded 4-byte accesses in the same kernels.  recnow_autoint_route: host-only, for a direction (bwd 0 / 1): 0 the weights
 * (and the backward's weight-gradient accumulators) resident in LDS, 1 read (accumulated) through L2 because they do not fit.
 * ---------------------------------------------------------------------------------------------------------- */
int recnow_autoint_supported(int F, int D, int H, int d);
int recnow_autoint_route(int F, int D, int H, int d, int use_res, int bwd);
size_t recnow_autoint_workspace_bytes(int64_t B, int F, int D, int H, int d, int use_res);
int recnow_autoint_fwd(const float* const* fields, int64_t xstride, int F, int64_t B, int D, int H, int d, const float* Wq,
                       const float* Wk, const float* Wv, const float* Wr, int scaling, int relu, float* out, void* stream);
int recnow_autoint_bwd(const float* const* fields, int64_t xstride, float* const* dfields, int64_t dxstride, int F, int64_t B, int D,
                       int H, int d, const float* Wq, const float* Wk, const float* Wv, const float* Wr, int scaling, int relu,
                       const float* dout, float* dWq, float* dWk, float* dWv, float* dWr, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * AFMLayer (ABI 27): the attention-pooled pairwise interaction of AFM (Xiao et al. 2017, arXiv 1708.04617, section 3).
 * csrc/afm.hip.  fields / dfields as for recnow_autoint_*: DEVICE arrays of F device pointers, field f of sample b at
 * fields[f] + b * xstride, one row stride in floats for all fields, >= D.  A = attention_factor; W (D, A) row-major, b (A), h (A),
 * p (D) or NULL without the projection.  Pairs k = (i, j), i < j, in InnerPNN's i-major order:
 *   p_k = x_i * x_j;  z_k = W^T p_k + b;  e_k = <relu(z_k), h>;  a = softmax of e over the pairs (maximum subtracted);
 *   v = sum_k a_k p_k;  out[b] = <v, p> (out (B, 1)) with p, else out[b][0 .. D) = v (out (B, D) contiguous).
 * fp32 FMA on exact fp32 operands, the exponential through the hardware exp2; neither the pair products nor the hidden layer
 * leave the chip.  B == 0: RECNOW_OK without a launch.  recnow_afm_bwd (dout shaped like out) recomputes the chain from the
 * fields and writes every row of every dfields[f] once; the ReLU subgradient at 0 is 0.  dW, db, dh (and dp with p) are either
 * all given or all NULL; NULL: no weight-gradient work, no reduce launch, and ws is not read.  Otherwise fp32 partials per
 * workgroup (one wave over a contiguous chunk of samples) are combined in fp64 in a fixed tree: no float atomics, the same
 * input gives the same bits on every run.  recnow_afm_workspace_bytes =
 *   4 G n rounded up to 256 bytes, n = 4 ceil((D A + 2 A + D) / 4), G = max(1, min(ceil(B / 4), 4096, 32 MiB / (4 n))).
 * recnow_afm_supported: host-only, 1 for 2 <= F <= 64 and 1 <= D, A <= 64; other shapes: RECNOW_EUNSUPPORTED from _fwd / _bwd
 * (a single field has no pair: the layer answers it with zeros without a call).  16-byte accesses need widths and row strides
 * that are multiples of 4 floats and 16-byte aligned bases; anything else takes guarded 4-byte accesses in the same kernels.
 * recnow_afm_route: host-only, for a direction (bwd 0 / 1): 0, the one route built (one wave per sample, tiles in wave-private
 * LDS, weights through the scalar cache), or RECNOW_EUNSUPPORTED.
 * ---------------------------------------------------------------------------------------------------------- */
int recnow_afm_supported(int F, int D, int A);
int recnow_afm_route(int F, int D, int A, int bwd);
size_t recnow_afm_workspace_bytes(int64_t B, int F, int D, int A);
int recnow_afm_fwd(const float* const* fields, int64_t xstride, int F, int64_t B, int D, int A, const float* W, const float* b,
                   const float* h, const float* p, float* out, void* stream);
int recnow_afm_bwd(const float* const* fields, int64_t xstride, float* const* dfields, int64_t dxstride, int F, int64_t B, int D,
                   int A, const float* W, const float* b, const float* h, const float* p, const float* dout, float* dW, float* db,
                   float* dh, float* dp, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * In-batch sampled softmax (ABI 29): the retrieval loss of a two-tower model over in-batch negatives, csrc/in_batch_softmax.hip.
 * An addition; the reference has no such loss.  q, v: (B, D) fp32 with row strides ldq, ldv in floats (>= D).  ids (B) int64 or NULL,
 * log_q (B) fp32 or NULL, mask (B) uint8 or NULL (NULL: every row takes part).  With inv_tau = 1 / temperature:
 *   s_ij = <q_i, v_j> inv_tau - log_q[j];  row i takes part iff mask[i] != 0;  column j is a candidate of row i iff j == i, or
 *   mask[j] != 0 and not (remove_hits and ids and ids[j] == ids[i]);  l_i = lse_{j in C(i)} s_ij - s_ii.
 * recnow_ibs_fwd writes per row the statistic (row_max[i], row_logsum[i]) with lse_i = row_max[i] + row_logsum[i] (row_logsum the log
 * of the sum rescaled by the maximum: exactly 0 for a row whose only candidate is itself), row_pos[i] = s_ii and row_loss[i] = l_i
 * (rows that do not take part: NaN, NaN, NaN, 0), then loss[0] = the mean of l_i over the n taking-part rows (0 when n = 0) and
 * n_rows[0] = n, by a fixed-order fp64 reduction of one partial per workgroup.  No (B, B) memory: a workgroup keeps
 * recnow_ibs_tile(0) rows on chip and walks the other side in tiles of recnow_ibs_tile(1) rows, the logit tiles on
 * v_mfma_f32_32x32x2_f32 (exact fp32).  recnow_ibs_bwd recomputes the tiles and writes, each row once,
 *   dq_i = c sum_j (p_ij - [j == i]) v_j,   dv_j = c sum_{i takes part} (p_ij - [j == i]) q_i,   c = gout[0] inv_tau / n,
 * p_ij = exp(s_ij - lse_i) on candidates, 0 elsewhere; rows that do not take part get 0.  gout and n_rows are DEVICE scalars (nothing
 * synchronises); dq or dv may be NULL: that orientation is not launched.  Rows that do not take part may hold anything, NaN included.
 * No atomics: the same input gives the same bits on every run.  B == 0: RECNOW_OK without a launch (loss and n_rows are not written).
 * recnow_ibs_workspace_bytes = 16 ceil(B / recnow_ibs_tile(0)) for the forward (bwd = 0), 0 for the backward.
 * recnow_ibs_supported: host-only, 1 for B >= 0 and 1 <= D <= 128, else 0 (RECNOW_EUNSUPPORTED from _fwd / _bwd).
 * recnow_ibs_tile(which): 0 the rows a workgroup owns, 1 the rows of a streamed tile, 2 the D granule rows are padded to on chip.
 * 16-byte global accesses need D and the row stride multiples of 4 floats and a 16-byte aligned base (decided per tensor); anything
 * else takes guarded 4-byte accesses in the same kernels, with the same bits.  recnow_ibs_launches(orientation, vec): host-only count
 * of the launches so far of orientation 0 (forward), 1 (dq), 2 (dv) whose OWNER-side tensor took 16-byte (vec 1) or 4-byte (vec 0)
 * accesses; orientation + 4: the same for the streamed-side tensor.
 * ---------------------------------------------------------------------------------------------------------- */
int recnow_ibs_supported(int64_t B, int D);
size_t recnow_ibs_workspace_bytes(int64_t B, int D, int bwd);
int recnow_ibs_tile(int which);
int64_t recnow_ibs_launches(int orientation, int vec);
int recnow_ibs_fwd(const float* q, int64_t ldq, const float* v, int64_t ldv, const int64_t* ids, const float* log_q,
                   const uint8_t* mask, int64_t B, int D, float inv_tau, int remove_hits, float* row_max, float* row_logsum,
                   float* row_pos, float* row_loss, float* loss, float* n_rows, void* ws, size_t ws_bytes, void* stream);
int recnow_ibs_bwd(const float* q, int64_t ldq, const float* v, int64_t ldv, const int64_t* ids, const float* log_q,
                   const uint8_t* mask, int64_t B, int D, float inv_tau, int remove_hits, const float* row_max,
                   const float* row_logsum, const float* n_rows, const float* gout, float* dq, int64_t lddq, float* dv,
                   int64_t lddv, void* ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------------------
 * Extra negatives for the in-batch sampled softmax (C ABI 31): N rows on the item side that have no query row of their own -- uniformly
 * sampled items (mixed negative sampling), a memory bank of earlier steps' items, or the other ranks' items after an all-gather.
 * extra: (N, D) fp32 with row stride ld_extra (>= D); extra_ids (N) int64 or NULL -- given iff ids is; extra_log_q (N) fp32 or NULL;
 * extra_mask (N) uint8 or NULL (NULL: every extra is on).  Extra k is a candidate of row i iff row i takes part, extra_mask[k] != 0 and not
 * (remove_hits and ids and extra_ids[k] == ids[i]); it is never a positive.  s_{i,B+k} = <q_i, e_k> inv_tau - extra_log_q[k].  Everything
 * else is as recnow_ibs_fwd / _bwd state it, with C(i) the larger set; with N = 0 the two entries ARE those (same kernels, same bits).
 * The forward and dq stream the items and then, from a fresh tile, the extras through the same recnow_ibs_tile(1)-row LDS tile; the owners
 * are the B queries, so the workspace is recnow_ibs_workspace_bytes(B, D, 0) as before (16 bytes per forward workgroup) and no memory of
 * the library's is sized by N.  recnow_ibs_extra_bwd writes
 *   dq_i = c (sum_j (p_ij - [j == i]) v_j + sum_k p_{i,B+k} e_k),   dv as recnow_ibs_bwd,   de_k = c sum_{i takes part} p_{i,B+k} q_i
 * de: (N, D) with row stride ldde, written by a launch of its own that owns recnow_ibs_tile(0) extras per workgroup and streams the queries
 * with their saved statistic; extras with extra_mask 0 may hold anything (NaN included) and get 0.  Each of dq, dv, de may be NULL: that
 * orientation is not launched.  Backward workspace: 0.  B == 0: RECNOW_OK without a launch (de is not written).
 * RECNOW_EINVAL: N < 0, ld_extra < D, a missing pointer with N > 0, ids without extra_ids or the reverse; RECNOW_EUNSUPPORTED: N > 2^30.
 * recnow_ibs_extra_launches(which, vec): host-only count of the launches so far of which 0 (a forward with an extra segment), 1 (a dq with
 * one), 2 (de, counted by its owner side) and 3 (de, by its streamed side); vec 1: 16-byte accesses were used for the extras (which 0 to 2)
 * or the queries (which 3), vec 0: guarded 4-byte accesses.  Negative outside those ranges.  These launches are not in recnow_ibs_launches;
 * the dv launch of recnow_ibs_extra_bwd is.
 * ---------------------------------------------------------------------------------------------------------- */
int64_t recnow_ibs_extra_launches(int which, int vec);
int recnow_ibs_extra_fwd(const float* q, int64_t ldq, const float* v, int64_t ldv, const int64_t* ids, const float* log_q,
                         const uint8_t* mask, int64_t B, int D, const float* extra, int64_t ld_extra, const int64_t* extra_ids,
                         const float* extra_log_q, const uint8_t* extra_mask, int64_t N, float inv_tau, int remove_hits,
                         float* row_max, float* row_logsum, float* row_pos, float* row_loss, float* loss, float* n_rows, void* ws,
                         size_t ws_bytes, void* stream);
int recnow_ibs_extra_bwd(const float* q, int64_t ldq, const float* v, int64_t ldv, const int64_t* ids, const float* log_q,
                         const uint8_t* mask, int64_t B, int D, const float* extra, int64_t ld_extra, const int64_t* extra_ids,
                         const float* extra_log_q, const uint8_t* extra_mask, int64_t N, float inv_tau, int remove_hits,
                         const float* row_max, const float* row_logsum, const float* n_rows, const float* gout, float* dq,
                         int64_t lddq, float* dv, int64_t lddv, float* de, int64_t ldde, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * (ABI 32) In-batch retrieval ranks: for every taking-part row, how many candidates score above its positive.  Arguments, taking part,
 * candidates C(i) and logits are those of recnow_ibs_extra_fwd (N = 0: no extras, extra may be NULL).  batch_candidates != 0: C(i) as in
 * the loss.  batch_candidates == 0 (full-corpus evaluation): batch item i is row i's positive and no batch column is a candidate of any
 * row; the candidates are the extras alone, with extra_mask and the id-hit rule.  With pos = s_ii and C'(i) = C(i) \ {i}, per row:
 *   n_candidates[i] = |C'(i)|,   n_greater[i] = #{j in C'(i): not (s_ij <= pos)},   n_equal[i] = #{j in C'(i): s_ij == pos},
 * (B) int64 each, and row_pos[i] = pos (float).  A NaN logit or a NaN pos counts as greater.  Rows that do not take part get 0, 0, 0
 * and NaN and may hold anything; so may masked extras.  pos and every candidate logit are results of one and the same fp32 expression
 * on the same MFMA chain: a candidate whose row and log_q are bit-identical to the positive's is counted equal wherever it stands, and
 * row_pos is, bit for bit, the row_pos of recnow_ibs_fwd / recnow_ibs_extra_fwd.  One launch of the loss's kernel template: a workgroup
 * owns recnow_ibs_tile(0) queries, reads its own two item tiles for pos, then walks the items (batch_candidates != 0 only) and the extras
 * in tiles of recnow_ibs_tile(1) rows.  No workspace, no atomics, each row written once: the same input gives the same bits on every
 * run.  B == 0: RECNOW_OK without a launch.  Errors as recnow_ibs_extra_fwd; RECNOW_EINVAL for a NULL output or inv_tau <= 0.
 * recnow_ibs_rank_launches(which, vec): host-only count of the rank launches so far whose queries (which 0), items (which 1) or extras
 * (which 2; launches with N > 0 only) took 16-byte (vec 1) or guarded 4-byte (vec 0) accesses; which 3: launches that walked the item
 * segment (vec 1) or left it to the two tiles of the positives (vec 0).  Negative outside those ranges.  Rank launches are in neither
 * recnow_ibs_launches nor recnow_ibs_extra_launches.
 * ---------------------------------------------------------------------------------------------------------- */
int64_t recnow_ibs_rank_launches(int which, int vec);
int recnow_ibs_rank(const float* q, int64_t ldq, const float* v, int64_t ldv, const int64_t* ids, const float* log_q,
                    const uint8_t* mask, int64_t B, int D, const float* extra, int64_t ld_extra, const int64_t* extra_ids,
                    const float* extra_log_q, const uint8_t* extra_mask, int64_t N, float inv_tau, int remove_hits,
                    int batch_candidates, int64_t* n_greater, int64_t* n_equal, int64_t* n_candidates, float* row_pos, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * (ABI 33) In-batch top-K candidates: for every taking-part row, the K candidates that score highest -- hard-negative mining from the
 * batch or a memory bank, top-K retrieval of a corpus.  Arguments, checks, taking part, C'(i) = C(i) \ {i}, the logits and
 * batch_candidates are those of recnow_ibs_rank (N = 0 allowed); the positive is never in the list.
 * Order: candidate a stands before candidate b iff a's score is NaN and b's is not, or score_a > score_b, or the scores compare equal
 * (or both are NaN) and index_a < index_b.  -0.0 and 0.0 tie; NaN is greatest.  The order is total: the result is a function of the
 * candidate set alone.  An index addresses cat(items, extras) in both candidate modes: batch column j is j, extra k is B + k.
 * Row i of scores (B, K; float, leading dimension ld_scores >= K) and indices (B, K; int64, ld_indices >= K) holds the first
 * min(K, |C'(i)|) candidates in that order, then the fill: score -inf, index -1.  A candidate whose logit is -inf carries its index and
 * stands before the fill.  n_candidates[i] = |C'(i)| as recnow_ibs_rank writes it.  Rows that do not take part get all fill and 0 and
 * may hold anything; so may masked extras.  A score is the result of the one fp32 expression recnow_ibs_rank compares and
 * recnow_ibs_fwd exponentiates.  One launch of the loss's kernel template; the lists live in dynamic LDS (8 K + 4 bytes a row, 64 rows a
 * workgroup).  No workspace, no atomics, every output element written once: the same input gives the same bits on every run.
 * B == 0: RECNOW_OK without a launch.  Errors as recnow_ibs_rank; RECNOW_EINVAL for K < 1, a NULL output or a leading dimension below
 * K; RECNOW_EUNSUPPORTED for K > recnow_ibs_topk_max_k() (128).
 * recnow_ibs_topk_launches(which, vec): the census of recnow_ibs_rank_launches, for these launches alone; which 3: launches that walked
 * the item segment (vec 1) or left it out (vec 0).  Top-K launches are in no other census.
 * ---------------------------------------------------------------------------------------------------------- */
int recnow_ibs_topk_max_k(void);
int64_t recnow_ibs_topk_launches(int which, int vec);
int recnow_ibs_topk(const float* q, int64_t ldq, const float* v, int64_t ldv, const int64_t* ids, const float* log_q,
                    const uint8_t* mask, int64_t B, int D, const float* extra, int64_t ld_extra, const int64_t* extra_ids,
                    const float* extra_log_q, const uint8_t* extra_mask, int64_t N, float inv_tau, int remove_hits,
                    int batch_candidates, int K, float* scores, int64_t ld_scores, int64_t* indices, int64_t ld_indices,
                    int64_t* n_candidates, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Measurement hook (bench.py): per-launch HIP-event timing of the GEMM kernels on the launch stream.
 * recnow_prof_enable(capacity > 0) arms `capacity` launch slots, (0) disables.  recnow_prof_collect synchronises and
 * returns per-kernel-family totals in HOST arrays of 16 entries indexed by tag: 1 = k_gemm<128,128>, 2 = k_gemm<128,160>,
 * 3 = k_gemm<256,64>, 4 = k_gemm<256,32>, 5 = k_gemm_shortk, 6 = k_mix_mid_fwd, 7 = k_mix_mid_bwd, 8 = k_gemm_split, 9 = the fused GEMM1,
 * 10 / 11 = k_mix_tile_fwd / _bwd, 12 = k_gemm<64,128> (csrc/prof.hpp): launches, total
 * milliseconds, total algorithmic flops (2*M*N*K*batch) and (bytes_host, may be NULL) total algorithmic HBM bytes: every
 * operand read once, every output written once, read-modify-write outputs twice.
 * ---------------------------------------------------------------------------------------------------------- */
int recnow_prof_enable(int capacity);
/* Time only every n-th GEMM launch (default 1 = all): the two timing events around a launch cost ~2 us of stream
 * serialisation each; with n coprime to the launches per step every launch position is sampled equally often. */
int recnow_prof_sample_every(int n);
int recnow_prof_collect(int* count_host, double* ms_host, double* flops_host, double* bytes_host);
/* The recorded launches one by one instead of per-tag totals: tag_host / t0_ms_host / t1_ms_host (HOST arrays of `capacity` entries) get
 * the tag and the interval of every record, in milliseconds after the first record's start; returns the number written or a negative
 * code; synchronises and rewinds like recnow_prof_collect.  After recnow_prof_sample_every(1) the records are EVERY hooked launch plus
 * the phase tags 13 (grouping), 14 (loss stage), 15 (packs, layer-end reductions): the timeline from which a caller tells overlapping
 * launches of two streams apart. */
int recnow_prof_intervals(int* tag_host, double* t0_ms_host, double* t1_ms_host, int capacity);
/* (ABI 6) Entries of the per-tag arrays recnow_prof_collect fills -- size the host arrays from this -- and the number of records that found the pool full
 * since the last recnow_prof_enable / the last call (non-zero: the totals and intervals under-report; re-arm with a larger capacity). */
int recnow_prof_tag_count(void);
int recnow_prof_dropped(void);

/* HIP events owned through the C ABI (timing disabled): the layer_events_host of recnow_dcn_mix_score_bwd.  A host framework
 * whose event type is created lazily (torch.cuda.Event) cannot hand a handle over before the first record. */
int recnow_event_create(void** event_out);
int recnow_event_destroy(void* event);
int recnow_event_record(void* event, void* stream);
int recnow_stream_wait_event(void* stream, void* event);
/* x[0..n) *= 1 / (count[0] + eps), count a DEVICE scalar: the in-place normalisation of a reduced gradient bucket by the global
 * pair count (pairwise_loss_from_batch.py:125-126, P + 1e-10) without a host round trip.  x 16-byte aligned.
 * stats_out (optional, 2 floats): receives (loss_sum[0] / (count[0] + eps), count[0]) = the mean loss the reference returns
 * (pairwise_loss_from_batch.py:279) and the pair count, from the same launch. */
int recnow_scale_by_inv_count(float* x, int64_t n, const float* count, float eps, const float* loss_sum, float* stats_out,
                              void* stream);

/* ----------------------------------------------------------------------------------------------------------
 * attention_by_softmax (C ABI 34): masked multi-head softmax target attention of a padded history against H queries per sample.
 * An addition; the reference has no softmax attention.  user: (B, L, D) fp32, keys and values; query: (B, H, D) fp32; lengths: (B) int32
 * or NULL (values below 0 act as 0, above L as L); mask: (B, L) uint8 or NULL (non-zero: a key).  Position l is a key of sample b iff
 * l < lengths[b] and mask[b][l] != 0 (a NULL argument does not restrict).  scale finite and > 0.  Over the keys K(b):
 *   s_hl = scale <query[b,h], user[b,l]>;   a_hl = exp(s_hl - m_h) / S_h,  m_h = max_l s_hl,  S_h = sum_l exp(s_hl - m_h)
 *   out[b,h] = sum_l a_hl user[b,l]   (B, H, D);     stat[b,h] = (m_h, log2 S_h)   (B, H, 2):  lse = m_h + ln 2 * log2 S_h
 * (the logarithm to base 2, the hardware's own: a sum that is a power of two comes back exactly).  A sample without a key gets out = 0
 * and stat = (-inf, -inf).  Positions outside K(b) are kept out by selects: they may hold NaN or inf, and positions at or beyond the
 * length are not read.  recnow_attention_softmax_bwd recomputes the scores from user, query and stat and writes, with dc = dout (B, H, D),
 *   ds_hl = a_hl (<dc_h, x_l> - <dc_h, out_h>);   duser[b,l] = sum_h (a_hl dc_h + scale ds_hl q_h)  (0 outside K(b));
 *   dquery[b,h] = scale sum_l ds_hl x_l.
 * duser or dquery NULL: that output is not computed (both NULL: no launch).  No workspace, no atomics, no LDS; every row is written once,
 * the same input gives the same bits on every run.  B == 0: RECNOW_OK without a launch.  D > 256 or H > 8: RECNOW_EUNSUPPORTED;
 * recnow_attention_softmax_supported: host-only, 1 for L >= 0, 1 <= D <= 256, 1 <= H <= 8, else 0.
 * recnow_attention_softmax_route: host-only, which kernel _fwd (which = 0) / _bwd (which = 1) launch.  align_mask: one bit per tensor that
 * starts OFF a 16-byte boundary: 1 user, 2 query, 4 out, and for the backward 8 dout, 16 duser, 32 dquery.  Returns 200000 + 100 CPL + HB
 * for the vector kernels k_as_v4_fwd / _bwd<CPL, HB> (D = 4 CPL, CPL in {1, 2, 4, 8, 16}, every tensor aligned), 100000 + 100 GS + HB for the
 * guarded kernels k_as_fwd / _bwd<GS, HB> (GS = 16 / 32 / 64 lanes per sample for D <= 16 / <= 32 / <= 256); HB in {1, 2, 4, 8} is H rounded
 * up to a power of two.  0 for B = 0; RECNOW_EUNSUPPORTED as above; RECNOW_EINVAL: which outside {0, 1}, B < 0, L < 0, D < 1, H < 1, or an
 * align_mask outside the direction's bits.
 * recnow_attention_softmax_tile(which): 0 the samples per wave of the vector route, 1 the float4 pieces of a sample per loop trip, 2 the
 * lanes per sample; anything else RECNOW_EINVAL.
 * ---------------------------------------------------------------------------------------------------------- */
int recnow_attention_softmax_supported(int L, int D, int H);
int recnow_attention_softmax_route(int which, int64_t B, int L, int D, int H, int align_mask);
int recnow_attention_softmax_tile(int which);
int recnow_attention_softmax_fwd(const float* user, const float* query, const int32_t* lengths, const uint8_t* mask, int64_t B, int L, int D,
                                 int H, float scale, float* out, float* stat, void* stream);
int recnow_attention_softmax_bwd(const float* user, const float* query, const int32_t* lengths, const uint8_t* mask, const float* out,
                                 const float* stat, const float* dout, int64_t B, int L, int D, int H, float scale, float* duser,
                                 float* dquery, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RECNOW_H_ */
