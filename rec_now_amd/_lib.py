"""ctypes binding of librecnow_hip.so (the C ABI declared in include/recnow.h).

There is deliberately NO CPU fallback: if the shared library is missing, or a tensor is not on the GPU, the call
raises.  torch is used only for device memory, streams and autograd plumbing.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('RECNOW_LIB_PATH') or os.path.join(_HERE, 'librecnow_hip.so')      # override: A/B runs of two builds (tools/)

_c = ctypes
_P, _I, _L, _F, _Z = _c.c_void_p, _c.c_int, _c.c_int64, _c.c_float, _c.c_size_t


class CrossDesc(ctypes.Structure):
    """recnow_cross_desc of include/recnow.h (passed by value)."""
    _fields_ = [
        ('ids', _P * 4), ('dtype', _c.c_int32 * 4), ('len', _c.c_int32 * 4), ('batch1', _c.c_int32 * 4),
        ('n_inputs', _c.c_int32), ('sep_len', _c.c_int32), ('sep_word', _c.c_uint32), ('default_len', _c.c_int32),
        ('n_alt', _c.c_int32 * 4), ('lit_len', (_c.c_int32 * 8) * 4), ('lit_words', ((_c.c_uint64 * 3) * 8) * 4),
        ('default_words', _c.c_uint64 * 12), ('default_buckets', _c.c_int64 * 16),
    ]


# name -> (restype, argtypes); kept in the order of include/recnow.h
SIGNATURES = {
    'recnow_abi_version': (_I, []),
    'recnow_key_words': (_I, [_I]),
    'recnow_group_keys': (_I, [_P, _I, _L, _P, _P, _P]),
    'recnow_group_segments_workspace_bytes': (_Z, [_L, _I]),
    'recnow_group_segments': (_I, [_P, _P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_pairwise_workspace_bytes': (_Z, [_L]),
    'recnow_pair_count': (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _I, _P, _P, _P, _P, _Z, _P]),
    'recnow_pair_offsets': (_I, [_P, _L, _P, _P, _Z, _P]),
    'recnow_pair_emit': (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _P, _P, _P, _L, _P, _Z, _P]),
    'recnow_pair_bpr_fwdbwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _F, _F, _I, _P, _P, _P, _Z, _P]),
    'recnow_pair_bpr_onepass': (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _F, _I, _P, _P, _P, _P, _Z, _P]),
    'recnow_pair_scale_grad': (_I, [_P, _P, _P, _F, _L, _P, _P]),
    'recnow_pair_table_count': (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _I, _P, _I, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_pair_table_bpr_fwdbwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _P, _I, _P, _F, _F, _I, _P, _P, _P, _Z, _P]),
    'recnow_pair_kind_fwdbwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _F, _P, _I, _P, _F, _F, _I, _P, _P, _P, _Z, _P]),
    'recnow_pair_lambda_workspace_bytes': (_Z, [_L]),
    'recnow_pair_lambda_terms': (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_pair_lambda_fwdbwd': (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _F, _I, _P, _F, _F, _I, _P, _P, _P, _Z, _P]),
    'recnow_pair_auc_workspace_bytes': (_Z, [_L]),
    'recnow_pair_auc_terms': (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _F, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_pair_auc_sorted_workspace_bytes': (_Z, [_L]),
    'recnow_pair_auc_sorted_terms': (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _F, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_pairwise_loss_workspace_bytes': (_Z, [_L, _I]),
    'recnow_pairwise_loss': (_I, [_P, _I, _P, _P, _P, _L, _I, _F, _I, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_pairwise_small_supported': (_I, [_L, _I]),
    'recnow_group_pack_small': (_I, [_P, _I, _P, _P, _P, _L, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_bpr_loss_fwdbwd': (_I, [_P, _P, _P, _L, _F, _I, _P, _P, _P, _Z, _P]),
    'recnow_pair_mask_dense': (_I, [_P, _P, _P, _L, _I, _P, _P]),
    'recnow_occurance_power_weight': (_I, [_P, _P, _P, _L, _F, _P, _P]),
    'recnow_listwise_workspace_bytes': (_Z, [_L]),
    'recnow_listwise_segments': (_I, [_P, _P, _P, _P, _P, _L, _F, _F, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_listwise_loss_fwdbwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _P, _P]),
    'recnow_listwise_loss_workspace_bytes': (_Z, [_L, _I]),
    'recnow_listwise_loss': (_I, [_P, _I, _P, _P, _P, _L, _F, _F, _P, _P, _P, _Z, _P]),
    'recnow_listwise_dense': (_I, [_P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _P]),
    'recnow_listwise_dense_bwd': (_I, [_P, _P, _L, _P, _P]),
    'recnow_softmax_ce_rows_fwd': (_I, [_P, _P, _L, _L, _P, _P, _P, _P]),
    'recnow_softmax_ce_rows_bwd': (_I, [_P, _P, _P, _P, _P, _L, _L, _P, _P]),
    'recnow_listmle_workspace_bytes': (_Z, [_L]),
    'recnow_listmle_fwdbwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_approx_ndcg_workspace_bytes': (_Z, [_L]),
    'recnow_approx_ndcg_fwdbwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_fm_fwd': (_I, [_P, _I, _L, _I, _P, _P, _P]),
    'recnow_fm_bwd': (_I, [_P, _P, _I, _L, _I, _P, _P, _P]),
    'recnow_fm_route': (_I, [_I, _L, _I, _I, _I]),
    'recnow_gemm_workspace_bytes': (_Z, [_P]),
    'recnow_gemm': (_I, [_P, _P, _Z, _P]),
    'recnow_gemm_route': (_I, [_P, _Z, _P]),
    'recnow_set_gemm_precision': (_I, [_I]),
    'recnow_get_gemm_precision': (_I, []),
    'recnow_set_gemm_staging': (_I, [_I]),
    'recnow_get_gemm_staging': (_I, []),
    'recnow_multi_dense_workspace_bytes': (_Z, [_L, _I, _I, _I]),
    'recnow_multi_dense_fwd': (_I, [_P, _I, _P, _P, _L, _I, _I, _I, _I, _P, _P, _Z, _P]),
    'recnow_multi_dense_bwd': (_I, [_P, _I, _P, _P, _P, _L, _I, _I, _I, _I, _P, _P, _P, _P, _Z, _P]),
    'recnow_moe_mix_fwd': (_I, [_P, _P, _I, _L, _I, _I, _P, _P, _P]),
    'recnow_moe_mix_bwd': (_I, [_P, _P, _P, _I, _L, _I, _I, _P, _P, _I, _P]),
    'recnow_dcn_workspace_bytes': (_Z, [_L, _I, _I]),
    'recnow_dcn_fwd': (_I, [_P, _P, _P, _L, _I, _I, _I, _P, _P, _P]),
    'recnow_dcn_bwd': (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _I, _P, _P, _P, _P, _Z, _P]),
    'recnow_dcn_route': (_I, [_I, _L, _I, _I, _I, _I]),
    'recnow_dcn_step_workspace_bytes': (_Z, [_L, _I]),
    'recnow_dcn_step_fwd': (_I, [_P, _P, _P, _P, _L, _I, _I, _P, _P, _P]),
    'recnow_dcn_step_bwd': (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_dcn_mix_saved_bytes': (_Z, [_L, _I, _I, _I, _I]),
    'recnow_dcn_mix_workspace_bytes': (_Z, [_L, _I, _I, _I, _I]),
    'recnow_dcn_mix_fwd': (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _P, _Z, _P, _Z, _P, _I]),
    'recnow_dcn_mix_bwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _Z, _L, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P,
                                 _Z, _P, _P]),
    'recnow_dcn_mix_score_supported': (_I, [_L, _I, _I, _I, _I]),
    'recnow_dcn_mix_tile_route': (_I, [_L, _I, _I, _I, _I]),
    'recnow_dcn_mix_score_fwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _P, _Z, _P, _Z, _P, _I]),
    'recnow_dcn_mix_score_bwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _L, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P,
                                       _P, _P, _Z, _P, _P, _P]),
    'recnow_dcn_mix_step_workspace_bytes': (_Z, [_L, _I, _I, _I, _I, _I]),
    'recnow_dcn_mix_step': (_I, [_P, _I, _I, _I, _P]),
    'recnow_cin_saved_bytes': (_Z, [_L, _I, _I, _P, _I]),
    'recnow_cin_workspace_bytes': (_Z, [_L, _I, _I, _P, _I]),
    'recnow_cin_fwd': (_I, [_P, _P, _L, _I, _I, _P, _I, _I, _I, _P, _P, _Z, _P, _Z, _P]),
    'recnow_cin_bwd': (_I, [_P, _P, _P, _Z, _L, _I, _I, _P, _I, _I, _I, _P, _P, _P, _Z, _P]),
    'recnow_inner_pnn_fwd': (_I, [_P, _I, _L, _I, _P, _P]),
    'recnow_inner_pnn_bwd': (_I, [_P, _P, _I, _L, _I, _P, _P]),
    'recnow_inner_pnn_route': (_I, [_I, _L, _I, _I, _I]),
    'recnow_senet_squeeze': (_I, [_P, _P, _P, _I, _I, _L, _P, _I, _P]),
    'recnow_senet_scale_fwd': (_I, [_P, _P, _P, _I, _I, _L, _P, _P, _I, _P]),
    'recnow_senet_scale_bwd_w': (_I, [_P, _P, _P, _I, _I, _L, _P, _P, _I, _P]),
    'recnow_senet_scale_bwd_x': (_I, [_P, _P, _P, _I, _I, _L, _P, _P, _P, _I, _P]),
    'recnow_senet_route': (_I, [_I, _L, _I, _I, _I]),
    'recnow_senet_grid': (_I, [_I, _L, _I, _I, _I]),
    'recnow_senet_fused_supported': (_I, [_I, _I, _I]),
    'recnow_senet_fused_workspace_bytes': (_Z, [_L, _I, _I]),
    'recnow_senet_fused_fwd': (_I, [_P, _I, _I, _L, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    'recnow_senet_fused_bwd': (_I, [_P, _P, _I, _I, _L, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_senet_fused_route': (_I, [_I, _L, _I, _I, _I, _I]),
    'recnow_senet_fused_grid': (_I, [_I, _L, _I, _I, _I, _I]),
    'recnow_attention_dot_fwd': (_I, [_P, _P, _L, _I, _I, _I, _P, _P, _P]),
    'recnow_attention_dot_bwd': (_I, [_P, _P, _P, _P, _L, _I, _I, _I, _P, _P, _P]),
    'recnow_attention_dot_route': (_I, [_I, _L, _I, _I, _I]),
    'recnow_attention_dnn_workspace_bytes': (_Z, [_L, _I, _I, _I, _P, _I]),
    'recnow_attention_dnn_fwd': (_I, [_P, _P, _L, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _Z, _P]),
    'recnow_attention_dnn_bwd': (_I, [_P, _P, _L, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_focal_loss_workspace_bytes': (_Z, [_L]),
    'recnow_focal_loss_fwd': (_I, [_P, _P, _L, _F, _F, _P, _P, _P, _Z, _P]),
    'recnow_focal_loss_bwd': (_I, [_P, _P, _L, _F, _F, _I, _P, _P, _F, _P, _P]),
    'recnow_slot_targets': (_I, [_P, _I, _P, _I, _P, _L, _P, _P, _L, _P, _P]),
    'recnow_embed_pool_fwd': (_I, [_P, _I, _L, _P, _P, _P, _L, _I, _I, _I, _P, _P, _P]),
    'recnow_embed_pool_bwd_weights': (_I, [_P, _I, _L, _P, _P, _P, _P, _L, _I, _I, _I, _P, _P]),
    'recnow_embed_unique': (_I, [_P, _P, _P, _P, _P, _L, _P, _P, _P, _P]),
    'recnow_embed_rows_bwd_workspace_bytes': (_Z, [_L, _I]),
    'recnow_embed_rows_bwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P, _P, _P, _Z, _P]),
    'recnow_embed_rows_bwd_direct': (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _L, _I, _I, _P, _L, _P, _Z, _P]),
    'recnow_embed_scatter_rows': (_I, [_P, _P, _L, _I, _L, _P, _P, _P]),
    'recnow_slot_max_count': (_I, [_P, _I, _L, _L, _I, _P, _P]),
    'recnow_slot_fetch': (_I, [_P, _I, _L, _P, _I, _P, _L, _I, _I, _L, _F, _P, _P, _P, _P, _P]),
    'recnow_slot_fetch_bwd': (_I, [_P, _P, _L, _I, _I, _P, _P]),
    'recnow_slot_embed_fwd': (_I, [_P, _I, _L, _P, _I, _L, _P, _I, _P, _L, _I, _I, _F, _P, _P, _P, _P, _P, _P, _L, _P]),
    'recnow_slot_pool_fwd': (_I, [_P, _P, _I, _P, _L, _I, _I, _I, _I, _P, _P, _P, _P]),
    'recnow_slot_pool_bwd': (_I, [_P, _P, _P, _L, _I, _I, _I, _I, _P, _P]),
    'recnow_hash_ids_host': (_I, [_P, _I, _L, _P, _I, _I, _L, _P]),
    'recnow_hash_bytes_host': (_I, [_P, _P, _L, _P, _I, _I, _L, _P]),
    'recnow_hash_ids': (_I, [_P, _I, _L, _P, _I, _I, _L, _P, _P]),
    'recnow_hash_embed_fwd': (_I, [_P, _I, _L, _L, _P, _I, _I, _L, _P, _I, _P, _I, _P, _P, _P, _P]),
    'recnow_hash_embed_bwd_weights': (_I, [_P, _P, _I, _L, _I, _P, _L, _L, _P, _P]),
    'recnow_cross_text_host': (_I, [CrossDesc, _L, _I, _P, _P]),
    'recnow_cross_hash_ids_host': (_I, [CrossDesc, _L, _P, _I, _I, _L, _P]),
    'recnow_cross_text': (_I, [CrossDesc, _L, _I, _P, _P, _P]),
    'recnow_cross_hash_ids': (_I, [CrossDesc, _L, _P, _I, _I, _L, _P, _P]),
    'recnow_cross_hash_embed_fwd': (_I, [CrossDesc, _L, _P, _I, _I, _L, _P, _I, _P, _I, _P, _P, _P, _P]),
    'recnow_star_dense_workspace_bytes': (_Z, [_L, _I, _I]),
    'recnow_star_dense_fwd': (_I, [_P, _P, _I, _I, _F, _P, _P, _L, _I, _I, _I, _P, _P]),
    'recnow_star_dense_bwd': (_I, [_P, _P, _I, _I, _F, _P, _P, _P, _L, _I, _I, _I, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_sparse_gnn_workspace_bytes': (_Z, [_L, _I, _I, _I, _I]),
    'recnow_sparse_gnn_fwd': (_I, [_P, _P, _I, _I, _I, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    'recnow_sparse_gnn_bwd': (_I, [_P, _P, _I, _I, _I, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P, _Z, _P]),
    'recnow_sparse_gnn_dense_workspace_bytes': (_Z, [_I, _I, _I, _I]),
    'recnow_sparse_gnn_dense_fwd': (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _Z, _P]),
    'recnow_sparse_gnn_dense_bwd': (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P, _Z, _P]),
    'recnow_reduce_axis_workspace_bytes': (_Z, [_L, _L, _L]),
    'recnow_reduce_axis_fwd': (_I, [_P, _L, _L, _L, _I, _P, _P, _Z, _P]),
    'recnow_reduce_axis_bwd': (_I, [_P, _P, _P, _L, _L, _L, _I, _P, _P]),
    'recnow_pad_axis': (_I, [_P, _I, _L, _L, _L, _L, _L, _P, _P]),
    'recnow_elem_weight_fwd': (_I, [_P, _P, _P, _L, _I, _I, _P, _P]),
    'recnow_elem_weight_bwd': (_I, [_P, _P, _P, _P, _P, _P, _L, _I, _I, _P, _P, _P]),
    'recnow_can_supported': (_I, [_I, _P, _I, _I]),
    'recnow_can_fwd': (_I, [_P, _P, _P, _L, _L, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    'recnow_can_bwd': (_I, [_P, _P, _P, _P, _L, _L, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    'recnow_bilinear_supported': (_I, [_I, _I, _I]),
    'recnow_bilinear_route': (_I, [_I, _I, _I, _I]),
    'recnow_bilinear_workspace_bytes': (_Z, [_L, _I, _I, _I]),
    'recnow_bilinear_fwd': (_I, [_P, _I, _L, _I, _I, _P, _P, _P]),
    'recnow_bilinear_bwd': (_I, [_P, _P, _I, _L, _I, _I, _P, _P, _P, _P, _Z, _P]),
    'recnow_autoint_supported': (_I, [_I, _I, _I, _I]),
    'recnow_autoint_route': (_I, [_I, _I, _I, _I, _I, _I]),
    'recnow_autoint_workspace_bytes': (_Z, [_L, _I, _I, _I, _I, _I]),
    'recnow_autoint_fwd': (_I, [_P, _L, _I, _L, _I, _I, _I, _P, _P, _P, _P, _I, _I, _P, _P]),
    'recnow_autoint_bwd': (_I, [_P, _L, _P, _L, _I, _L, _I, _I, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_afm_supported': (_I, [_I, _I, _I]),
    'recnow_afm_route': (_I, [_I, _I, _I, _I]),
    'recnow_afm_workspace_bytes': (_Z, [_L, _I, _I, _I]),
    'recnow_afm_fwd': (_I, [_P, _L, _I, _L, _I, _I, _P, _P, _P, _P, _P, _P]),
    'recnow_afm_bwd': (_I, [_P, _L, _P, _L, _I, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_ibs_supported': (_I, [_L, _I]),
    'recnow_ibs_workspace_bytes': (_Z, [_L, _I, _I]),
    'recnow_ibs_tile': (_I, [_I]),
    'recnow_ibs_launches': (_L, [_I, _I]),
    'recnow_ibs_fwd': (_I, [_P, _L, _P, _L, _P, _P, _P, _L, _I, _F, _I, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_ibs_bwd': (_I, [_P, _L, _P, _L, _P, _P, _P, _L, _I, _F, _I, _P, _P, _P, _P, _P, _L, _P, _L, _P, _Z, _P]),
    'recnow_ibs_extra_launches': (_L, [_I, _I]),
    'recnow_ibs_extra_fwd': (_I, [_P, _L, _P, _L, _P, _P, _P, _L, _I, _P, _L, _P, _P, _P, _L, _F, _I, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    'recnow_ibs_extra_bwd': (_I, [_P, _L, _P, _L, _P, _P, _P, _L, _I, _P, _L, _P, _P, _P, _L, _F, _I, _P, _P, _P, _P, _P, _L, _P, _L, _P, _L,
                                  _P, _Z, _P]),
    'recnow_ibs_rank_launches': (_L, [_I, _I]),
    'recnow_ibs_rank': (_I, [_P, _L, _P, _L, _P, _P, _P, _L, _I, _P, _L, _P, _P, _P, _L, _F, _I, _I, _P, _P, _P, _P, _P]),
    'recnow_ibs_topk_launches': (_L, [_I, _I]),
    'recnow_ibs_topk_max_k': (_I, []),
    'recnow_ibs_topk': (_I, [_P, _L, _P, _L, _P, _P, _P, _L, _I, _P, _L, _P, _P, _P, _L, _F, _I, _I, _I, _P, _L, _P, _L, _P, _P]),
    'recnow_attention_softmax_supported': (_I, [_I, _I, _I]),
    'recnow_attention_softmax_route': (_I, [_I, _L, _I, _I, _I, _I]),
    'recnow_attention_softmax_tile': (_I, [_I]),
    'recnow_attention_softmax_fwd': (_I, [_P, _P, _P, _P, _L, _I, _I, _I, _F, _P, _P, _P]),
    'recnow_attention_softmax_bwd': (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _F, _P, _P, _P]),
    'recnow_prof_enable': (_I, [_I]),
    'recnow_prof_sample_every': (_I, [_I]),
    'recnow_prof_collect': (_I, [_P, _P, _P, _P]),
    'recnow_prof_intervals': (_I, [_P, _P, _P, _I]),
    'recnow_prof_tag_count': (_I, []),
    'recnow_prof_dropped': (_I, []),
    'recnow_event_create': (_I, [_P]),
    'recnow_event_destroy': (_I, [_P]),
    'recnow_event_record': (_I, [_P, _P]),
    'recnow_stream_wait_event': (_I, [_P, _P]),
    'recnow_scale_by_inv_count': (_I, [_P, _L, _P, _F, _P, _P, _P]),
}


class GemmDesc(ctypes.Structure):
    """recnow_gemm_desc of include/recnow.h (host struct of device pointers and sizes)."""
    _fields_ = [
        ('A', _P), ('A2', _P), ('lda', _L), ('a_batch_stride', _L), ('a_trans', _I), ('a_mode', _I), ('a_act', _I), ('a_pad', _I),
        ('B', _P), ('B2', _P), ('ldb', _L), ('b_batch_stride', _L), ('b_trans', _I), ('b_mode', _I), ('b_act', _I), ('b_pad', _I),
        ('C', _P), ('ldc', _L), ('c_batch_stride', _L),
        ('M', _I), ('N', _I), ('K', _I), ('batch', _I),
        ('bias', _P), ('bias_batch_stride', _L),
        ('emul', _P), ('lde', _L), ('e_batch_stride', _L),
        ('act', _I), ('act_cols', _I), ('e_mode', _I), ('e_act', _I), ('accumulate', _I), ('a_hq', _I), ('b_hq', _I), ('a_ld2', _L), ('b_ld2', _L), ('c_trans', _I),
        ('sp_bx', _P), ('sp_cx', _P), ('sp_bx_ks', _L), ('sp_bx_rs', _L), ('sp_cx_ms', _L), ('sp_cx_rs', _L), ('sp_r', _I), ('sp_pad', _I),
        ('eu_p', _P), ('eu_q', _P), ('eu_pms', _L), ('eu_qrs', _L), ('eu_qns', _L), ('eu_r', _I), ('eu_pad', _I), ('prof_flops', ctypes.c_double),
        ('C2', _P), ('ldc2', _L), ('E2', _P), ('lde2', _L), ('c2_mode', _I), ('c2_pad', _I), ('as_in', _P), ('as_out', _P),
        ('E3', _P), ('lde3', _L), ('rv', _P), ('cv', _P), ('hv', _P), ('hp', _P), ('hp_ld', _I), ('hp_pad', _I), ('k_valid', _I), ('k_pad', _I), ('c_perm_s', _I), ('c_perm_pad', _I),
        ('mid_V', _P), ('mid_T1', _P), ('mid_T2', _P), ('mid_T2g', _P), ('mid_ld', _L), ('mid_act_outer', _I), ('mid_pad', _I),
        ('E4', _P), ('E5', _P), ('E6', _P),
    ]


class GemmRouteInfo(ctypes.Structure):
    """recnow_gemm_route_info of include/recnow.h: the planned route of a recnow_gemm call."""
    _fields_ = [(n, ctypes.c_int32) for n in (
        'family', 'bm', 'bn', 'bk', 'a_kc', 'b_kc', 'edge', 'a2k', 'b2k', 'xf', 'bp', 'pair', 'ep', 'c2_mode', 'planes',
        'splitk', 'kchunk', 'grid_x', 'grid_y', 'grid_z', 'xcd_remap', 'tail_pairs', 'reduce_variant', 'reduce_blocks', 'tag')]


ABI_VERSION = 35 # the recnow_abi_version() the SIGNATURES above were written for (csrc/abi.hip)

class StepDesc(ctypes.Structure):
    """recnow_dcn_mix_step_desc of include/recnow.h."""
    _fields_ = [
        ('B', _L), ('D', _I), ('S', _I), ('N', _I), ('L', _I), ('act_inner', _I), ('act_outer', _I), ('group_dtype', _I),
        ('only_use_wrong_order_pair', _I), ('reduce_mean', _I), ('factor', _F),
        ('x', _P), ('labels', _P), ('groups', _P), ('mask', _P),
        ('U_host', _P), ('V_host', _P), ('W_host', _P), ('bias_host', _P), ('gate_host', _P), ('head_w', _P), ('head_b', _P),
        ('scores', _P), ('loss', _P), ('n_pair', _P), ('stats', _P), ('dx', _P),
        ('dU_host', _P), ('dV_host', _P), ('dW_host', _P), ('dbias_host', _P), ('dgate_host', _P), ('dhead_w', _P), ('dhead_b', _P),
        ('ws', _P), ('ws_bytes', _Z), ('stream2', _P), ('layer_events_host', _P), ('B_pad', _L),
    ]


_ERR = {-1: 'RECNOW_EINVAL', -2: 'RECNOW_EWORKSPACE', -3: 'RECNOW_EUNSUPPORTED'}
_lib = None


def load():
    """Load librecnow_hip.so once.  torch must already be imported (it is, above) so that both share one HIP runtime."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'rec_now_amd: %s not found. Build it with `python -c "import __graft_entry__ as g; g.build()"` '
                '(hipcc --offload-arch=gfx950). There is no CPU fallback.' % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        lib.recnow_abi_version.restype = _I
        have = lib.recnow_abi_version()
        if have != ABI_VERSION:      # a stale build (or a foreign one through RECNOW_LIB_PATH) would take shifted arguments silently
            raise RuntimeError('rec_now_amd: %s exports C ABI version %d, these bindings were written for version %d; rebuild it with '
                               '`python -c "import __graft_entry__ as g; g.build()"`' % (LIB_PATH, have, ABI_VERSION))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError here = symbol missing from the .so
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError('%s failed: %s' % (what, _ERR.get(rc, 'hipError_t %d' % rc)))


def call(name, *args):
    rc = getattr(load(), name)(*args)
    check(rc, name)


def require_gpu(t, what='tensor'):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor, got %s' % (what, type(t)))
    if not t.is_cuda:
        raise RuntimeError('rec_now_amd computes only on the GPU (hand-written gfx950 kernels); %s is on %s. '
                           'Move it with .cuda(); there is no CPU fallback.' % (what, t.device))
    return t


def f32c(t, what='tensor'):
    """contiguous fp32 CUDA tensor (no copy when already so)."""
    require_gpu(t, what)
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    return t.contiguous()


def aligned_fields(tensors, vector_route):
    """The field tensors of a list-of-tensor call, each on a 16-byte boundary when the call takes a float4 route.  recnow_fm_fwd / _bwd (D % 4 == 0)
    and the Gram kernels of InnerPNN read float4 pieces of every field and do not test its base pointer; a contiguous view that starts a few floats into
    a larger buffer passes f32c and is not aligned.  Such a field is replaced by a copy (clone(): a fresh allocation); every other tensor is returned as
    it is, and nothing is touched when the route is scalar."""
    if not vector_route:
        return list(tensors)
    return [t if t.data_ptr() % 16 == 0 else t.clone() for t in tensors]


def ptr(t):
    if t is None:
        return None
    return _P(t.data_ptr())


# torch.cuda.current_stream() resolves its device through torch.cuda.is_available() (an os.getenv and a Stream object per call): 20-70 us
# of host time on every entry point.  The raw accessors return the same hipStream_t of the current device in well under a microsecond.
_RAW_STREAM = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_RAW_DEVICE = getattr(torch._C, '_cuda_getDevice', None)


def stream():
    if _RAW_STREAM is not None and _RAW_DEVICE is not None:
        return _P(_RAW_STREAM(_RAW_DEVICE()))
    return _P(torch.cuda.current_stream().cuda_stream)


_side_streams = {}


def side_stream(device):
    """One extra HIP stream per device for the entry points that accept a `stream2` (concurrent independent GEMMs)."""
    key = (device.type, device.index)
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device=device)
    return _P(_side_streams[key].cuda_stream)


def workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


_SMALL_CONST = {}


def const_array(values, dtype, device):
    """Small read-only device array holding `values`, uploaded once per distinct content: the tables of the list-of-tensor
    kernels (base pointers, field widths, column offsets) repeat from step to step -- the caching allocator hands the same
    blocks back -- and every fresh upload is a host-blocking copy of a few hundred bytes."""
    key = (str(device), dtype, tuple(values))
    hit = _SMALL_CONST.get(key)
    if hit is None:
        if len(_SMALL_CONST) >= 1024:
            _SMALL_CONST.clear()
        host = torch.tensor(key[2], dtype=dtype)
        # the host copy is kept with the entry: a stream capture records this upload with the host address
        hit = (host.to(device, non_blocking=True), host)
        _SMALL_CONST[key] = hit
    return hit[0]


def block_ptr_array(buf, n_blocks):
    """Device array of the base pointers of the n_blocks equal, consecutive blocks of the contiguous tensor `buf`
    (buf[f] for f < n_blocks) -- without creating n_blocks views first."""
    base, step = buf.data_ptr(), buf.numel() // n_blocks * buf.element_size()
    return const_array([base + f * step for f in range(n_blocks)], torch.int64, buf.device)


def ptr_array(tensors, device):
    """Device array of base pointers (int64) for list-of-tensor kernels."""
    return const_array([t.data_ptr() for t in tensors], torch.int64, device)
