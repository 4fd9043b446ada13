#include "common.hpp"
// Bumped whenever an exported signature or recnow_gemm_desc changes incompatibly; rec_now_amd/_lib.py refuses a library whose
// version differs from the one its SIGNATURES table was written for.  2: recnow_prof_collect (4 arrays), recnow_embed_pool_fwd
// (V), recnow_gemm_desc (second outputs, side products); 3 (round 3): recnow_dcn_mix_step + its descriptor, recnow_pairwise_loss,
// recnow_listwise_loss, the packed weights kept in recnow_dcn_mix_saved_bytes; 4 (round 5): recnow_dcn_mix_step_desc.B_pad (ragged per-rank
// batches on the fast route), recnow_dcn_mix_tile_route; 5 (round 5, second session): recnow_set_gemm_staging / recnow_get_gemm_staging (new symbols: a
// version-4 build would fail to bind them); 6 (round 6): recnow_prof_tag_count / recnow_prof_dropped, the split-precision piece planes in
// recnow_dcn_mix_saved_bytes; 7: recnow_star_dense_fwd / _bwd / _workspace_bytes (StarDenseLayer, StackedDenseLayer); 8: recnow_attention_dnn_fwd / _bwd /
// _workspace_bytes (attention_by_dnn); 9: recnow_sparse_gnn_fwd / _bwd / _workspace_bytes (SparseGNNLayer); 10: recnow_hash_ids / _ids_host / _bytes_host, recnow_hash_embed_fwd /
// _bwd_weights, recnow_embed_rows_bwd_direct (MultiHashLayer, FastMultiHashLayer); 11: recnow_slot_max_count, recnow_slot_fetch / _fetch_bwd, recnow_slot_embed_fwd,
// recnow_slot_pool_fwd / _pool_bwd (fetch_single_slot, embedding_single_slot, pool_slots); 12: recnow_reduce_axis_fwd / _bwd / _workspace_bytes, recnow_pad_axis,
// recnow_elem_weight_fwd / _bwd (PoolingLayer, FixLengthLayer, gather_embedding_element_wise_weight); 13: recnow_can_fwd / _bwd / _supported (CANLayer);
// 14: recnow_cross_desc, recnow_cross_text / _hash_ids (+ _host twins), recnow_cross_hash_embed_fwd (CartesianProductLayer);
// 15: recnow_sparse_gnn_dense_fwd / _bwd / _workspace_bytes (SparseGNNLayer, the dense MFMA route); 16: RECNOW_KEY_INF_EQUAL in the key dtype of
// recnow_key_words / recnow_group_keys / recnow_listwise_loss (a version-15 build answers it with RECNOW_EINVAL), fp64 per-list sums (seg_lse, seg_ysum,
// seg_psum, seg_pdot) in recnow_listwise_segments / _loss_fwdbwd / _dense; 17: recnow_pair_table_count / recnow_pair_table_bpr_fwdbwd
// (LabelPairWeightTable: the fused pairwise loss with per-label-pair weights); 18: recnow_pair_kind_fwdbwd (hinge, squared-hinge and margin-logistic
// pair terms on the fused route); 19: recnow_pair_lambda_terms / _fwdbwd / _workspace_bytes (the NDCG pair weight on the fused route, in-batch NDCG);
// 20: recnow_pair_auc_terms / _workspace_bytes (in-batch GAUC from exact pair counts); 21: recnow_dcn_route (the route choice of recnow_dcn_fwd / _bwd, queryable);
// 22: recnow_pair_auc_sorted_terms / _sorted_workspace_bytes (in-batch GAUC and AUC by sort and per-class prefix counts);
// 23: recnow_listmle_fwdbwd / _workspace_bytes (in-batch ListMLE on segmented fp64 log-sum-exp scans);
// 24: recnow_approx_ndcg_fwdbwd / _workspace_bytes (in-batch ApproxNDCG on the pair-walk skeletons);
// 25: recnow_bilinear_fwd / _bwd / _supported / _route / _workspace_bytes (BilinearInteractionLayer);
// 26: recnow_autoint_fwd / _bwd / _supported / _route / _workspace_bytes (InteractingLayer);
// 27: recnow_afm_fwd / _bwd / _supported / _route / _workspace_bytes (AFMLayer);
// 28: recnow_gemm_route / recnow_gemm_route_info (the planned route of recnow_gemm, queryable);
// 29: recnow_ibs_fwd / _bwd / _supported / _workspace_bytes / _tile / _launches (the in-batch sampled-softmax retrieval loss);
// 30: recnow_fm_route, recnow_inner_pnn_route, recnow_attention_dot_route (the kernel choice of FM, InnerPNN and attention_by_dot_product, queryable);
// 31: recnow_ibs_extra_fwd / _extra_bwd / _extra_launches (extra negatives for the in-batch sampled softmax: sampled items, a bank, other ranks);
// 32: recnow_ibs_rank / _rank_launches (in-batch retrieval ranks: recall@K, NDCG@K, MRR and mean rank from per-row counts).
// 33: recnow_ibs_topk / _topk_max_k / _topk_launches (in-batch top-K candidates: hard-negative mining and top-K retrieval of a corpus).
// 34: recnow_attention_softmax_fwd / _bwd / _supported / _route / _tile (attention_by_softmax: masked multi-head softmax target attention).
// 35: recnow_senet_route / _grid, recnow_senet_fused_route / _fused_grid (the kernel choice and the grid of every SENET entry, queryable).
extern "C" int recnow_abi_version(void) { return 35; }
