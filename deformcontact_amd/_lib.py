"""ctypes binding of ``libdeformcontact_hip.so`` (the C ABI in ``include/deformcontact.h``).

There is deliberately NO fallback: if the library is missing or fails to load,
every op raises.  The CPU oracle under ``oracle/`` is test infrastructure and is
never imported from here.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libdeformcontact_hip.so")

_lib = None

_vp = c_void_p
_SIGNATURES = {
    "dc_version": (c_int, []),
    "dc_last_error": (c_char_p, []),
    "dc_stream_capture_id": (c_int64, [_vp]),
    "dc_csr_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "dc_csr_build": (c_int, [_vp, c_int64, c_int64, c_int, c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                             _vp, c_int64, _vp]),
    "dc_graph_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "dc_graph_build": (c_int, [_vp, c_int64, c_int64, c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                               _vp, _vp, c_int64, _vp]),
    "dc_graph_build_parts": (c_int, [POINTER(_vp), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), c_int,
                                     c_int64, c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c_int64,
                                     _vp]),
    "dc_graph_build_plan": (c_int, [c_int64, c_int64, c_int, POINTER(c_int), POINTER(c_int)]),
    "dc_graph_build_segmented": (c_int, [_vp, c_int64, c_int64, POINTER(c_int64), POINTER(c_int64), c_int,
                                         _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dc_hop_chain_image_bytes": (c_int64, [c_int64]),
    "dc_graph_build_segmented_image": (c_int, [_vp, c_int64, c_int64, POINTER(c_int64), POINTER(c_int64), c_int,
                                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dc_graph_build_segmented_loops": (c_int, [_vp, c_int64, c_int64, POINTER(c_int64), POINTER(c_int64), c_int,
                                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dc_attn_flash_prep": (c_int, [_vp, c_int64, c_int64, _vp, _vp, _vp]),
    "dc_attn_flash_ds": (c_int, [_vp, c_int64, _vp, _vp, c_int64, _vp, _vp, _vp, _vp, _vp, _vp, c_int64, c_int64,
                                 c_int64, c_int64, _vp, _vp, c_int64, _vp, _vp, _vp, _vp]),
    "dc_tag_linear_fwd_h2p_corr": (c_int, [_vp, c_int64, _vp, _vp, _vp, _vp, c_int64, c_int64, c_int64, c_int64, _vp, _vp,
                                           _vp]),
    "dc_tag_linear_bwd_dw_h2_corr": (c_int, [_vp, c_int64, _vp, _vp, POINTER(_vp), POINTER(c_int64), c_int, POINTER(_vp),
                                             c_int, c_int64, c_int, _vp, c_int64, c_int64, c_int64, c_int64, _vp, _vp,
                                             _vp]),
    "dc_attn_flash_fwd": (c_int, [_vp, c_int64, _vp, _vp, _vp, _vp, _vp, c_int64, c_int64, c_int64, c_int64, _vp,
                                  c_int64, _vp, _vp]),
    "dc_hop_chain_max_nodes": (c_int64, []),
    "dc_hop_chain_lds_request": (c_int64, []),
    "dc_hop_chain_f32": (c_int, [_vp, _vp, _vp, _vp, c_int64, POINTER(c_int64), c_int, _vp, c_int64, c_int64, c_int64,
                                 c_int, c_int, c_int, _vp, c_int, _vp]),
    "dc_hop_chain_image_f32": (c_int, [_vp, _vp, _vp, _vp, c_int64, POINTER(c_int64), c_int, _vp, c_int64, c_int64,
                                       c_int64, c_int, c_int, c_int, _vp, c_int, _vp, _vp]),
    "dc_spmm_f32_bias_act": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_int, _vp, c_int64, c_int64, c_int64, _vp]),
    "dc_colsum_workspace_bytes": (c_int64, [c_int64, c_int64, c_int]),
    "dc_mask_colsum_f32": (c_int, [_vp, c_int64, _vp, c_int64, _vp, c_int64, c_int64, c_int64, _vp, c_int64, _vp, c_int,
                                   _vp]),
    "dc_gat_alpha_fwd": (c_int, [_vp, c_int64, _vp, _vp, _vp, _vp, c_int64, c_int64, _vp]),
    "dc_gat_alpha_bwd": (c_int, [_vp, c_int64, _vp, _vp, _vp, _vp, _vp, c_int64, c_int64, c_int64, _vp, c_int64, _vp, _vp,
                                 c_int, _vp]),
    "dc_spmm_f32_pack": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_int64, c_int64, c_int64, c_int64, c_int64, _vp]),
    "dc_spmm_f32_pack_wprep": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_int64, c_int64, c_int64, c_int64, c_int64,
                                       POINTER(_vp), c_int, _vp, _vp]),
    "dc_spmm_f32_window": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_int64,
                                   c_int64, c_int64, _vp]),
    "dc_spmm_f32_rowmax_window": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_int64,
                                          c_int64, _vp, c_int, c_int64, _vp]),
    "dc_tag_grouped_weight_prep": (c_int, [POINTER(_vp), c_int, c_int, c_int64, c_int64, POINTER(_vp),
                                           POINTER(_vp), POINTER(_vp), POINTER(_vp), _vp]),
    "dc_tag_grouped_fwd_h2p": (c_int, [_vp, c_int64, c_int, POINTER(c_int64), POINTER(c_int64), c_int64,
                                       POINTER(_vp), POINTER(_vp), c_int, _vp, c_int64, c_int64, c_int64, _vp,
                                       POINTER(_vp), _vp]),
    "dc_tag_grouped_mask_grad": (c_int, [POINTER(_vp), POINTER(c_int64), c_int, POINTER(c_int64),
                                         POINTER(c_int64), c_int64, _vp, c_int64, _vp, c_int64, c_int64, _vp,
                                         _vp, _vp]),
    "dc_tag_grouped_bwd_dw_workspace_bytes": (c_int64, [POINTER(c_int64), c_int, c_int64, c_int64, c_int]),
    "dc_tag_grouped_bwd_dw_h2": (c_int, [_vp, c_int64, POINTER(_vp), POINTER(c_int64), c_int, c_int,
                                         POINTER(c_int64), POINTER(c_int64), c_int64, POINTER(_vp),
                                         POINTER(_vp), c_int, _vp, c_int64, c_int64, c_int64, _vp, _vp, _vp]),
    "dc_generic_dense_launches": (c_int64, [c_int]),
    "dc_kernel_trace": (None, [c_int]),
    "dc_kernel_trace_dump": (c_int64, [c_char_p, c_int64]),
    "dc_launch_sites_dump": (c_int64, [c_char_p, c_int64]),
    "dc_launch_coverage": (None, [c_int]),
    "dc_launch_reached_dump": (c_int64, [c_char_p, c_int64]),
    "dc_hash_i64": (c_int, [_vp, c_int64, _vp, _vp]),
    "dc_morton_codes": (c_int, [_vp, c_int64, c_int64, POINTER(c_float), POINTER(c_float), _vp, _vp]),
    "dc_morton_order_workspace_bytes": (c_int64, [c_int64]),
    "dc_morton_order": (c_int, [_vp, c_int64, c_int64, _vp, _vp, _vp, c_int64, _vp]),
    "dc_relabel_edges": (c_int, [_vp, c_int64, _vp, c_int64, _vp, _vp]),
    "dc_gather_rows": (c_int, [_vp, c_int64, _vp, _vp, c_int64, c_int64, c_int64, _vp]),
    "dc_invert_perm": (c_int, [_vp, _vp, _vp, c_int64, _vp]),
    "dc_neighbors_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "dc_neighbors_fill": (c_int, [_vp, c_int64, c_int64, _vp, _vp, c_int64, c_int64, _vp, c_int, c_float, c_int, c_int,
                                  _vp, _vp, _vp, c_int64, _vp]),
    "dc_neighbors_compact_workspace_bytes": (c_int64, [c_int64]),
    "dc_neighbors_compact": (c_int, [_vp, c_int, _vp, c_int64, c_int, _vp, c_int64, _vp, c_int64, _vp]),
    "dc_neighbors_nd_fill": (c_int, [_vp, c_int64, c_int64, _vp, _vp, c_int64, c_int64, _vp, c_int64, c_int, c_int,
                                     _vp, _vp, _vp]),
    "dc_spmm_f32": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_int64,
                            c_int64, _vp]),
    "dc_spmm_bf16": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_int64,
                             c_int64, c_int, _vp]),
    "dc_tag_linear_fwd_bf16": (c_int, [_vp, c_int64, _vp, _vp, c_int, _vp, c_int64, c_int, c_int64, c_int64,
                                       c_int64, _vp]),
    "dc_tag_mask_grad_bf16": (c_int, [_vp, c_int64, c_int, _vp, c_int64, c_int, _vp, c_int64, c_int64, c_int64, _vp]),
    "dc_tag_linear_bwd_dw_bf16_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64, c_int]),
    "dc_tag_linear_bwd_dw_bf16": (c_int, [_vp, c_int64, _vp, c_int64, c_int, POINTER(_vp), _vp, c_int, _vp, c_int64,
                                          c_int64, c_int64, c_int64, _vp]),
    "dc_to_bf16": (c_int, [POINTER(_vp), c_int, c_int64, c_int64, c_int64, _vp, c_int64, _vp]),
    "dc_contact_loss_workspace_bytes": (c_int64, [c_int64]),
    "dc_contact_loss": (c_int, [_vp, _vp, _vp, _vp, _vp, c_int64, _vp, c_int64, c_int64, c_int64, _vp, _vp,
                                _vp, _vp, c_int64, _vp]),
    "dc_tag_linear_fwd": (c_int, [POINTER(_vp), POINTER(c_int64), POINTER(_vp), c_int, _vp, c_int,
                                  _vp, c_int64, c_int64, c_int64, c_int64, _vp]),
    "dc_tag_linear_bwd_dx": (c_int, [_vp, c_int64, _vp, c_int64, POINTER(_vp), c_int,
                                     POINTER(_vp), POINTER(c_int64), c_int64, c_int64, c_int64,
                                     _vp]),
    "dc_tag_linear_fwd_split": (c_int, [POINTER(_vp), POINTER(c_int64), POINTER(_vp), c_int, _vp,
                                        c_int, _vp, c_int64, c_int64, c_int64, c_int64, c_int, _vp]),
    "dc_tag_linear_bwd_dx_split_workspace_bytes": (c_int64, [c_int64, c_int64, c_int]),
    "dc_tag_linear_bwd_dx_split": (c_int, [_vp, c_int64, _vp, c_int64, POINTER(_vp), c_int,
                                           POINTER(_vp), POINTER(c_int64), _vp, c_int64, c_int64,
                                           c_int64, c_int64, c_int, _vp]),
    "dc_tag_linear_bwd_dw_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64, c_int]),
    "dc_tag_linear_bwd_dw": (c_int, [_vp, c_int64, _vp, c_int64, POINTER(_vp), POINTER(c_int64),
                                     c_int, POINTER(_vp), c_int, c_int64, _vp, c_int, _vp, c_int64,
                                     c_int64, c_int64, c_int64, _vp]),
    "dc_tag_linear_bwd_dw_split": (c_int, [_vp, c_int64, _vp, c_int64, POINTER(_vp),
                                           POINTER(c_int64), c_int, POINTER(_vp), c_int, c_int64,
                                           _vp, c_int, _vp, c_int64, c_int64, c_int64, c_int64,
                                           c_int, _vp]),
    "dc_tag_linear_fwd_h2": (c_int, [POINTER(_vp), POINTER(c_int64), POINTER(_vp), c_int, _vp,
                                     c_int, _vp, c_int64, c_int64, c_int64, c_int64, _vp, _vp, _vp]),
    "dc_tag_linear_bwd_dx_h2": (c_int, [_vp, c_int64, _vp, c_int64, POINTER(_vp), c_int,
                                        POINTER(_vp), POINTER(c_int64), _vp, c_int64, c_int64,
                                        c_int64, c_int64, _vp, _vp, _vp]),
    "dc_tag_linear_bwd_dw_h2": (c_int, [_vp, c_int64, _vp, c_int64, POINTER(_vp),
                                        POINTER(c_int64), c_int, POINTER(_vp), c_int, c_int64,
                                        _vp, c_int, _vp, c_int64, c_int64, c_int64, c_int64,
                                        _vp, _vp, _vp]),
    "dc_tag_mask_grad": (c_int, [_vp, c_int64, _vp, c_int64, _vp, c_int64, c_int64, c_int64, _vp, _vp, _vp]),
    "dc_tag_transpose_weights": (c_int, [POINTER(_vp), c_int, c_int64, c_int64, _vp, _vp]),
    "dc_tag_linear_fwd_h2p_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64]),
    "dc_tag_linear_fwd_h2p": (c_int, [_vp, c_int64, _vp, _vp, c_int, _vp, c_int64, c_int64, c_int64, c_int64,
                                      _vp, _vp, _vp, c_int64, _vp]),
    "dc_tag_linear_fwd_h2p_exp": (c_int, [_vp, c_int64, _vp, _vp, c_int64, c_int64, c_int64, c_int64, _vp, _vp, _vp,
                                          c_int64, _vp]),
    "dc_tag_weight_prep": (c_int, [POINTER(_vp), c_int, c_int64, c_int64, _vp, _vp, _vp, _vp, _vp]),
    "dc_tag_weight_prep_zero": (c_int, [POINTER(_vp), c_int, c_int64, c_int64, _vp, _vp, _vp, _vp, _vp, c_int64, _vp]),
    "dc_rowabsmax_f32": (c_int, [_vp, c_int64, c_int64, c_int64, _vp, _vp]),
    "dc_tag_weight_rowmax": (c_int, [POINTER(_vp), c_int, c_int64, c_int64, _vp, _vp]),
    "dc_spmm_f32_rowmax": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_int64,
                                   c_int64, _vp, c_int, _vp]),
    "dc_tag_pack_input": (c_int, [_vp, c_int64, _vp, c_int64, c_int64, c_int64, c_int64, c_int64, _vp]),
    "dc_tag_pack_weights": (c_int, [POINTER(_vp), c_int, _vp, c_int64, c_int64, c_int64, _vp]),
    "dc_tag_linear_fwd_narrow_ok": (c_int, [c_int64, c_int, c_int64, c_int64]),
    "dc_tag_linear_fwd_narrow": (c_int, [_vp, c_int64, POINTER(_vp), c_int, c_int64, _vp, c_int, _vp, c_int64, c_int64,
                                         c_int64, c_int64, _vp]),
    "dc_tag_narrow_wimage": (c_int, [POINTER(_vp), c_int, c_int64, c_int64, _vp, _vp]),
    "dc_tag_linear_fwd_narrow_img": (c_int, [_vp, c_int64, _vp, _vp, c_int, _vp, c_int64, c_int64, c_int64, c_int64, _vp]),
    "dc_attn_softmax_rows": (c_int, [_vp, c_int64, c_int64, c_int64, c_int64, _vp, _vp]),
    "dc_attn_exp_rows": (c_int, [_vp, c_int64, c_int64, c_int64, c_int64, _vp, _vp]),
    "dc_attn_ds_rows": (c_int, [_vp, _vp, c_int64, c_int64, c_int64, _vp, _vp, _vp]),
    "dc_adam_flat": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_float, c_float, c_float, c_float,
                             c_int, _vp]),
    "dc_compose_perm": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp]),
    "dc_gat_edge_softmax_fwd": (c_int, [_vp, _vp, _vp, _vp, c_float, _vp, c_int64, _vp]),
    "dc_gat_edge_softmax_bwd": (c_int, [_vp, _vp, _vp, _vp, c_float, _vp, _vp, _vp, _vp, c_int64,
                                        _vp]),
    "dc_sddmm_f32": (c_int, [_vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_int64, _vp]),
    "dc_segment_sum_f32": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp]),
    "dc_gather_f32": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp]),
    "dc_gat_alpha_heads_fwd": (c_int, [_vp, c_int64, _vp, _vp, _vp, _vp, c_int64, c_int64, c_int64, _vp]),
    "dc_gat_edge_softmax_heads_fwd": (c_int, [_vp, _vp, _vp, _vp, c_float, _vp, c_int64, c_int64, _vp]),
    "dc_spmm_f32_heads_bias_act": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_int, c_int, _vp, c_int64, c_int64,
                                           c_int64, c_int64, _vp]),
    "dc_sddmm_f32_heads": (c_int, [_vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_int64, c_int64, _vp]),
    "dc_gat_edge_softmax_heads_bwd": (c_int, [_vp, _vp, _vp, _vp, c_float, _vp, _vp, _vp, _vp, c_int64, c_int64,
                                              _vp]),
    "dc_segment_sum_f32_heads": (c_int, [_vp, _vp, _vp, _vp, c_int64, c_int64, _vp]),
    "dc_gather_f32_heads": (c_int, [_vp, _vp, _vp, _vp, c_int64, c_int64, _vp]),
    "dc_spread_heads_f32": (c_int, [_vp, c_int64, _vp, c_int64, c_int64, c_int64, c_int64, _vp]),
    "dc_gat_alpha_heads_bwd": (c_int, [_vp, c_int64, _vp, _vp, _vp, _vp, _vp, c_int64, c_int64, c_int64, c_int64, _vp,
                                       c_int64, _vp, _vp, c_int, _vp]),
    "dc_gat_edge_attr_fwd": (c_int, [_vp, _vp, _vp, c_int64, _vp, c_int, c_float, _vp, _vp, c_int64, c_int64, c_int64,
                                     c_int64, _vp]),
    "dc_gat_edge_attr_softmax_fwd": (c_int, [_vp, _vp, _vp, _vp, _vp, c_float, _vp, c_int64, c_int64, _vp]),
    "dc_gat_edge_attr_softmax_bwd": (c_int, [_vp, _vp, _vp, _vp, _vp, c_float, _vp, _vp, _vp, _vp, c_int64, c_int64,
                                             _vp]),
    "dc_gat_edge_attr_bwd_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64]),
    "dc_gat_edge_attr_bwd": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, _vp, c_int, _vp, c_int64, _vp, c_int64, c_int64,
                                     c_int64, c_int64, c_int64, _vp, c_int64, _vp]),
    "dc_gatv2_softmax_fwd": (c_int, [_vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_float, _vp, c_int64, c_int64, c_int64,
                                     _vp]),
    "dc_gatv2_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64]),
    "dc_gatv2_softmax_bwd": (c_int, [_vp, _vp, _vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_float, _vp, _vp, c_int64, _vp,
                                     c_int, _vp, c_int64, c_int64, c_int64, c_int64, _vp]),
    "dc_gatv2_source_bwd": (c_int, [_vp, _vp, _vp, _vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, _vp, c_float, _vp,
                                    c_int64, c_int64, c_int64, c_int64, _vp]),
    "dc_tconv_softmax_fwd": (c_int, [_vp, _vp, _vp, c_int64, _vp, c_int64, c_float, _vp, c_int64, c_int64, c_int64, _vp]),
    "dc_tconv_softmax_bwd": (c_int, [_vp, _vp, _vp, _vp, _vp, c_int64, c_float, _vp, _vp, c_int64, c_int64, c_int64,
                                     c_int64, _vp]),
    "dc_tconv_source_bwd": (c_int, [_vp, _vp, _vp, _vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, _vp, c_int64,
                                    c_int64, c_int64, c_int64, _vp]),
    "dc_sage_mean_fwd": (c_int, [_vp, _vp, _vp, c_int64, _vp, c_int64, c_int64, c_int64, _vp]),
    "dc_sage_mean_bwd": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_int64, c_int64, c_int64, _vp]),
    "dc_sage_max_fwd": (c_int, [_vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_int64, c_int64, _vp]),
    "dc_sage_max_bwd": (c_int, [_vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_int64,
                                c_int64, _vp]),
    "dc_gine_fwd": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_int64, _vp, _vp, c_int64, c_int64, c_int64, _vp]),
    "dc_gine_bwd_x": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_int64, _vp, _vp, c_int64, _vp, c_int64, c_int64,
                              c_int64, _vp]),
    "dc_gine_bwd_e": (c_int, [_vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_int64, c_int64,
                              c_int64, _vp]),
    "dc_edge_pair_fwd": (c_int, [_vp, _vp, _vp, c_int64, _vp, c_int64, c_int64, c_int64, c_int64, _vp]),
    "dc_edge_pair_bwd": (c_int, [_vp, _vp, _vp, _vp, _vp, c_int64, _vp, c_int64, c_int64, c_int64, _vp]),
    "dc_edge_reduce_fwd": (c_int, [_vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_int, c_int64, c_int64, _vp]),
    "dc_edge_reduce_bwd": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, _vp, c_int64, _vp, c_int64,
                                   c_int, c_int64, c_int64, c_int64, _vp]),
    "dc_cheb_norm": (c_int, [_vp, _vp, _vp, _vp, c_int, c_float, _vp, _vp, _vp, c_int64, _vp]),
    "dc_cheb_hop": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_float,
                            c_int, c_int, c_int64, c_int64, _vp]),
    "dc_gmm_weights": (c_int, [_vp, c_int64, _vp, _vp, _vp, c_int64, c_int64, c_int64, _vp]),
    "dc_gmm_fwd": (c_int, [_vp, _vp, _vp, _vp, _vp, c_int64, _vp, c_int64, c_int, c_int, _vp, c_int64, c_int64, c_int64,
                           c_int64, c_int64, _vp]),
    "dc_gmm_bwd_h": (c_int, [_vp, _vp, _vp, _vp, _vp, _vp, c_int64, _vp, c_int64, c_int64, c_int64, c_int64, c_int64,
                             _vp]),
    "dc_gmm_bwd_w": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_int64, c_int64, c_int64, _vp]),
    "dc_gmm_params_workspace_bytes": (c_int64, [c_int64, c_int64, c_int64]),
    "dc_gmm_bwd_params": (c_int, [_vp, _vp, _vp, c_int64, _vp, _vp, _vp, c_int64, _vp, _vp, _vp, c_int64, c_int64,
                                  c_int64, c_int64, _vp]),
    "dc_spline_basis": (c_int, [_vp, c_int64, _vp, _vp, c_int64, _vp, _vp, c_int64, c_int64, _vp]),
    "dc_spline_fwd": (c_int, [_vp, _vp, _vp, _vp, _vp, _vp, c_int64, _vp, c_int64, c_int, c_int, _vp, c_int64, c_int64,
                              c_int64, c_int64, c_int64, c_int64, _vp]),
    "dc_spline_bwd_h": (c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, c_int64, _vp, c_int64, c_int64, c_int64, c_int64,
                                c_int64, c_int64, _vp]),
    "dc_spline_bwd_b": (c_int, [_vp, _vp, _vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_int64, c_int64, c_int64,
                                c_int64, _vp]),
    "dc_spline_bwd_a": (c_int, [_vp, _vp, c_int64, _vp, _vp, c_int64, _vp, c_int64, c_int64, c_int64, _vp]),
    "dc_fps_resident_points": (c_int64, []),
    "dc_fps_workspace_bytes": (c_int64, [c_int64, c_int64]),
    "dc_fps": (c_int, [_vp, c_int64, c_int64, _vp, _vp, c_int64, c_int64, _vp, _vp, c_int64, _vp, c_int64, _vp]),
    "dc_knn_interpolate_fwd": (c_int, [_vp, c_int64, _vp, c_int64, _vp, c_int64, _vp, _vp, c_int, _vp, c_int64, _vp, _vp,
                                       c_int64, c_int64, c_int64, _vp]),
    "dc_knn_interpolate_bwd": (c_int, [_vp, _vp, _vp, _vp, _vp, c_int64, _vp, c_int64, c_int, c_int64, c_int64, c_int64,
                                       _vp]),
    "dc_pointnet_pair_fwd": (c_int, [_vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_int64, c_int64,
                                     c_int64, c_int64, c_int, c_int, _vp]),
    "dc_pointnet_pair_bwd": (c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, _vp,
                                     c_int64, c_int64, c_int64, c_int64, c_int64, c_int, _vp]),
    "dc_pointnet_reduce_bwd": (c_int, [_vp, _vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, _vp, c_int64, _vp,
                                       c_int64, c_int, c_int64, c_int64, c_int64, c_int64, c_int, _vp]),
    "dc_pool_fwd": (c_int, [_vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_int, c_int64, c_int64, c_int64, _vp]),
    "dc_pool_bwd": (c_int, [_vp, _vp, _vp, c_int64, _vp, c_int64, _vp, c_int64, _vp, c_int64, _vp, c_int64, c_int,
                            c_int64, c_int64, c_int64, _vp]),
}


class DeformContactLibraryError(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle.  Raises loudly when absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise DeformContactLibraryError(
                f"{SO_PATH} not found. Build it with `python -m deformcontact_amd.build` "
                "(hipcc --offload-arch=gfx950). deformcontact_amd has no CPU/PyTorch fallback.")
        try:
            handle = ctypes.CDLL(SO_PATH)
        except OSError as e:  # pragma: no cover
            raise DeformContactLibraryError(f"cannot load {SO_PATH}: {e}") from e
        for name, (res, args) in _SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                raise DeformContactLibraryError(
                    f"{SO_PATH} does not export {name}; rebuild the library") from e
            fn.restype, fn.argtypes = res, args
        _lib = handle
        if os.environ.get(COVERAGE_ENV):
            _start_coverage(os.environ[COVERAGE_ENV])
    return _lib


# Launch-site coverage of a whole run ("Launch sites"): with DC_LAUNCH_COVERAGE_FILE set when the
# library loads, every process (children that inherit the variable included) appends the sites it reached, one
# "site \t test id at the first reach" line each, to that file when it exits.
COVERAGE_ENV = "DC_LAUNCH_COVERAGE_FILE"


def _start_coverage(path: str) -> None:
    import atexit
    _lib.dc_launch_coverage(1)

    def _append():
        lines = [f"{site}\t{test}\n" for site, test in launch_reached().items()]
        if lines:
            with open(path, "a") as f:      # one write per process: appends of concurrent children do not interleave
                f.write("".join(lines))
    atexit.register(_append)


def _dump(fn) -> list:
    n = int(fn(None, 0))
    buf = ctypes.create_string_buffer(n + 1)
    fn(buf, n + 1)
    return buf.value.decode().splitlines()


def launch_site_files() -> dict:
    """``{site: source file}`` for every launch site the library was built with (no GPU needed).  A site is
    ``kernel text @ enclosing host function``; a templated launcher gives one site per instantiation."""
    out = {}
    for line in _dump(lib().dc_launch_sites_dump):
        src, _, site = line.partition("\t")
        out[site] = src
    return out


def launch_sites() -> list:
    """Every launch site of the library (see ``launch_site_files``)."""
    return list(launch_site_files())


def launch_coverage(on: bool) -> None:
    """Start / stop adding launched sites to the cumulative reached set (``dc_launch_coverage``)."""
    lib().dc_launch_coverage(1 if on else 0)


def launch_reached() -> dict:
    """``{site: PYTEST_CURRENT_TEST at its first launch}`` for the sites reached while coverage was on."""
    return {site: test for site, test, _ in _reached_rows()}


def _reached_rows():
    return [line.split("\t") for line in _dump(lib().dc_launch_reached_dump)]


def launch_site_counts() -> dict:
    """``{site: launches while coverage was on}`` for the reached sites; the difference around a call names exactly
    the sites that call launched, whatever ran earlier in the process."""
    return {site: int(n) for site, _, n in _reached_rows()}


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().dc_last_error()
        raise DeformContactLibraryError(
            f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def kernel_trace(on: bool) -> None:
    """Start (clearing the log) / stop the library's launch log (``dc_kernel_trace``)."""
    lib().dc_kernel_trace(1 if on else 0)


def kernel_trace_counts() -> dict:
    """``{kernel name: launches}`` recorded since ``kernel_trace(True)``."""
    n = int(lib().dc_kernel_trace_dump(None, 0))
    buf = ctypes.create_string_buffer(n + 1)
    lib().dc_kernel_trace_dump(buf, n + 1)
    out = {}
    for line in buf.value.decode().splitlines():
        name, _, cnt = line.rpartition(" ")
        out[name] = int(cnt)
    return out


def exported_names():
    return list(_SIGNATURES)
