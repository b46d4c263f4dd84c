"""ctypes binding of libnafp.so (include/nafp.h).

There is no CPU fallback: if the shared library is missing or a call fails, this
module raises.  `import torch` happens first on purpose: the HIP runtime torch
ships (soname libamdhip64.so.7) is then the one libnafp binds to, so device
pointers and streams are shared between torch and the library.
"""
import ctypes
import os

import torch  # noqa: F401  (must be loaded before libnafp; see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
# NAFP_LIB: load another build of the same ABI (kernel ablation experiments, tools/ablate.sh)
LIB_PATH = os.environ.get('NAFP_LIB') or os.path.join(_HERE, 'libnafp.so')

c_i64 = ctypes.c_int64
c_int = ctypes.c_int
c_float = ctypes.c_float
c_void_p = ctypes.c_void_p

# name -> (restype, argtypes); mirrors include/nafp.h one to one.
PROTOTYPES = {
    'nafp_abi_version': (c_int, []),
    'nafp_status_string': (ctypes.c_char_p, [c_int]),
    'nafp_last_hip_error': (c_int, []),
    'nafp_crc32c_host': (ctypes.c_uint32, [c_void_p, c_i64, ctypes.c_uint32]),
    'nafp_mel_filterbank_host': (c_int, [c_int, c_int, c_int, c_float, c_float, c_void_p]),
    'nafp_melspec_create': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int, c_float, c_float]),
    'nafp_melspec_create_ex': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_int]),
    'nafp_melspec_plan_host': (c_int, [c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_int, c_void_p]),
    'nafp_melspec_kernel': (c_int, [c_void_p]),
    'nafp_melspec_destroy': (c_int, [c_void_p]),
    'nafp_melspec_n_frames': (c_int, [c_void_p]),
    'nafp_melspec_n_mels': (c_int, [c_void_p]),
    'nafp_melspec_forward_f32': (c_int, [c_void_p, c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'nafp_melspec_forward_i16': (c_int, [c_void_p, c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'nafp_melspec_finish': (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_void_p]),
    'nafp_melspec_forward_windows_i16': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_void_p,
                                                 c_void_p, c_void_p]),
    'nafp_resample_geometry': (c_int, [c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                                       ctypes.POINTER(c_int)]),
    'nafp_resample_table_host': (c_int, [c_int, c_int, c_void_p]),
    'nafp_resample_n_out': (c_i64, [c_i64, c_int, c_int]),
    'nafp_resample_input_range': (c_int, [c_i64, c_i64, c_i64, c_int, c_int, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    'nafp_resample_check_pieces_host': (c_int, [c_int, c_int, c_void_p, c_i64, c_i64, c_i64]),
    'nafp_resample_create': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int]),
    'nafp_resample_destroy': (c_int, [c_void_p]),
    'nafp_resample_i16': (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_void_p]),
    'nafp_ingest_geometry': (c_int, [c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                                     ctypes.POINTER(c_int)]),
    'nafp_ingest_table_host': (c_int, [c_int, c_int, c_void_p]),
    'nafp_ingest_n_out': (c_i64, [c_i64, c_int, c_int]),
    'nafp_ingest_input_range': (c_int, [c_i64, c_i64, c_i64, c_int, c_int, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    'nafp_ingest_decode_host': (c_int, [c_int, c_void_p, c_i64, c_void_p]),
    'nafp_ingest_check_pieces_host': (c_int, [c_int, c_int, c_void_p, c_i64, c_i64, c_i64]),
    'nafp_ingest_create': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int]),
    'nafp_ingest_destroy': (c_int, [c_void_p]),
    'nafp_ingest_i16': (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_void_p]),
    'nafp_varispeed_geometry': (c_int, [ctypes.c_uint32, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'nafp_varispeed_table_host': (c_int, [ctypes.c_uint32, c_void_p]),
    'nafp_varispeed_n_out': (c_i64, [c_i64, ctypes.c_uint32]),
    'nafp_varispeed_input_range': (c_int, [c_i64, c_i64, c_i64, ctypes.c_uint32, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    'nafp_varispeed_check_pieces_host': (c_int, [ctypes.c_uint32, c_void_p, c_i64, c_i64, c_i64]),
    'nafp_varispeed_create': (c_int, [ctypes.POINTER(c_void_p), ctypes.c_uint32]),
    'nafp_varispeed_destroy': (c_int, [c_void_p]),
    'nafp_varispeed_i16': (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_void_p]),
    'nafp_codec_samples_per_block': (c_int, [c_int, c_int, c_int]),
    'nafp_codec_blocks_per_group': (c_int, [c_int, c_int, c_int]),
    'nafp_codec_decode_host': (c_int, [c_int, c_int, c_int, c_void_p, c_i64, c_void_p]),
    'nafp_codec_check_pieces_host': (c_int, [c_void_p, c_i64, c_i64, c_i64]),
    'nafp_codec_decode_i16': (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_void_p]),
    'nafp_flac_streaminfo_host': (c_int, [c_void_p, c_i64, c_void_p]),
    'nafp_flac_index_host': (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_i64]),
    'nafp_flac_decode_host': (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_void_p]),
    'nafp_flac_check_frames_host': (c_int, [c_void_p, c_i64, c_i64, c_i64]),
    'nafp_flac_decode': (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_void_p]),
    'nafp_encoder_create': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int]),
    'nafp_encoder_create_ex': (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int]),
    'nafp_encoder_norm': (c_int, [c_void_p]),
    'nafp_encoder_n_trainable': (c_int, [c_void_p]),
    'nafp_encoder_destroy': (c_int, [c_void_p]),
    'nafp_encoder_n_tensors': (c_int, [c_void_p]),
    'nafp_encoder_tensor_numel': (c_i64, [c_void_p, c_int]),
    'nafp_encoder_tensor_shape': (c_int, [c_void_p, c_int, ctypes.POINTER(c_i64)]),
    'nafp_encoder_flat_dim': (c_i64, [c_void_p]),
    'nafp_encoder_set_weights': (c_int, [c_void_p, ctypes.POINTER(c_void_p), c_void_p]),
    'nafp_encoder_workspace_bytes': (c_i64, [c_void_p, c_i64]),
    'nafp_encoder_forward': (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_void_p, c_int, c_void_p]),
    'nafp_encoder_forward_raw': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_i64, c_void_p, c_i64, c_void_p, c_void_p,
                                         c_int, c_void_p]),
    'nafp_encoder_conv0_numel': (c_i64, [c_void_p]),
    'nafp_encoder_conv0': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_i64, c_void_p, c_void_p, c_void_p]),
    'nafp_encoder_profile_enable': (c_int, [c_void_p, c_int]),
    'nafp_encoder_profile_count': (c_int, [c_void_p]),
    'nafp_encoder_profile_coarse': (c_int, [c_void_p, c_int]),
    'nafp_encoder_profile_read': (c_int, [c_void_p, c_int, c_void_p]),
    'nafp_conv_timeline': (c_int, [c_void_p, c_i64, c_int, c_int, c_int]),
    'nafp_conv_timeline_grid': (c_int, [c_void_p]),
    'nafp_conv_plan': (c_int, [c_int, c_int, c_int, c_i64, c_i64, c_int, c_i64, c_void_p, c_void_p, c_int]),
    'nafp_encoder_set_option': (c_int, [c_void_p, c_int, c_int]),
    'nafp_encoder_train_workspace_bytes': (c_i64, [c_void_p, c_i64]),
    'nafp_encoder_forward_train': (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_int, c_void_p]),
    'nafp_encoder_backward': (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_i64,
                                      ctypes.POINTER(c_void_p), c_int, c_void_p]),
    'nafp_encoder_grad_group_range': (c_int, [c_void_p, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'nafp_encoder_grad_group_wait': (c_int, [c_void_p, c_int, c_void_p]),
    'nafp_encoder_div_enc': (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_int, c_void_p]),
    'nafp_ntxent_workspace_bytes': (c_i64, [c_i64, c_i64]),
    'nafp_ntxent_forward': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int,
                                    c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p]),
    'nafp_specaug_apply': (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_int, c_void_p, c_float, c_void_p]),
    'nafp_specaug_apply_fill_dev': (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'nafp_specaug_mean_workspace_bytes': (c_i64, []),
    'nafp_specaug_mean': (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_void_p]),
    'nafp_specaug_apply_ex': (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_int, c_i64, c_void_p, c_void_p, c_i64, c_void_p, c_void_p]),
    'nafp_specaug_range': (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_void_p]),
    'nafp_l2_normalize_rows': (c_int, [c_void_p, c_i64, c_int, c_void_p, c_void_p]),
    'nafp_pack_embedding_grads': (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_i64, c_i64, c_int, c_void_p, c_void_p]),
    'nafp_cosine_decay_lr_host': (c_float, [c_float, c_i64, c_i64, c_float]),
    'nafp_cosine_decay_restarts_lr_host': (c_float, [c_float, c_i64, c_i64, c_float, c_float, c_float]),
    'nafp_adam_step': (c_int, [c_void_p, c_int, c_float, c_float, c_float, c_float, c_i64, c_void_p]),
    'nafp_lamb_workspace_bytes': (c_i64, [c_void_p, c_int]),
    'nafp_triplet_workspace_bytes': (c_i64, [c_i64, c_i64]),
    'nafp_triplet_forward': (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_i64, c_void_p]),
    'nafp_augment_rows': (c_int, [c_void_p, c_void_p, c_i64, c_int, c_void_p, c_void_p]),
    'nafp_aug_speedset_create': (c_int, [ctypes.POINTER(c_void_p), c_void_p, c_int]),
    'nafp_aug_speedset_destroy': (c_int, [c_void_p]),
    'nafp_augment_speed_check_host': (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_int]),
    'nafp_augment_rows_speed': (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_int, c_void_p, c_void_p]),
    'nafp_search_index_aux_floats': (c_i64, [c_i64]),
    'nafp_search_index_prepare': (c_int, [c_void_p, c_i64, c_int, c_void_p, c_void_p]),
    'nafp_search_workspace_bytes': (c_i64, [c_i64, c_i64, c_int]),
    'nafp_search_topk_l2': (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p,
                                    c_void_p, c_i64, c_void_p]),
    'nafp_search_topk_l2_excl': (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_i64, c_void_p]),
    'nafp_search_seq_scores': (c_int, [c_void_p, c_void_p, c_i64, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_int,
                                       c_void_p, c_void_p]),
    'nafp_search_seq_match': (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_int, c_void_p, c_int, c_void_p, c_void_p, c_i64, c_int,
                                      c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'nafp_search_identify': (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_int, c_void_p, c_int, c_void_p, c_void_p, c_i64, c_int,
                                     c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
    'nafp_search_identify_check_tracks_host': (c_int, [c_void_p, c_int, c_i64]),
    'nafp_search_identify_tempo': (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_int, c_void_p, c_int, c_void_p, c_void_p, c_i64, c_int,
                                           c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'nafp_ivf_bucket_workspace_bytes': (c_i64, [c_i64, c_int, c_int]),
    'nafp_ivf_bucket': (c_int, [c_void_p, c_int, c_i64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_void_p]),
    'nafp_ivf_kmeans_update': (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'nafp_ivf_residuals': (c_int, [c_void_p, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'nafp_ivf_pq_encode': (c_int, [c_void_p, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'nafp_ivf_probe': (c_int, [c_void_p, c_i64, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'nafp_ivf_flat_rows_bound': (c_i64, [c_i64, c_int]),
    'nafp_ivf_flat_lists': (c_int, [c_void_p, c_i64, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    'nafp_ivf_pq_lists': (c_int, [c_void_p, c_i64, c_int, c_void_p, c_void_p, c_void_p]),
    'nafp_ivf_search_workspace_bytes': (c_i64, [c_i64, c_int, c_int, c_int, c_int]),
    'nafp_ivf_flat_search': (c_int, [c_void_p, c_i64, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                     c_void_p, c_void_p, c_void_p, c_i64, c_void_p]),
    'nafp_ivf_pq_search': (c_int, [c_void_p, c_i64, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                   c_int, c_void_p, c_void_p, c_void_p, c_i64, c_void_p]),
    'nafp_ivf_pq_search_ex': (c_int, [c_void_p, c_i64, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                      c_int, c_void_p, c_void_p, c_int, c_void_p, c_i64, c_void_p]),
    'nafp_ivf_pq_adc_tables': (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_void_p, c_int, c_int, c_void_p, c_int, c_int,
                                       c_void_p, c_void_p]),
    'nafp_ivf_pq_residuals': (c_int, [c_void_p, c_i64, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'nafp_ivf_refine_encode': (c_int, [c_void_p, c_i64, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'nafp_ivf_pq_wide_workspace_bytes': (c_i64, [c_i64, c_int, c_int, c_int]),
    'nafp_ivf_pq_search_wide': (c_int, [c_void_p, c_i64, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                        c_int, c_void_p, c_void_p, c_int, c_void_p, c_i64, c_void_p]),
    'nafp_ivf_pqr_rerank': (c_int, [c_void_p, c_i64, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                    c_int, c_int, c_void_p, c_i64, c_int, c_void_p, c_void_p, c_void_p]),
    'nafp_ivf_pqr_search': (c_int, [c_void_p, c_i64, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_i64, c_int, c_int, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_int, c_void_p, c_i64, c_void_p]),
    'nafp_hnsw_default_max_expansions': (c_int, [c_int]),
    'nafp_hnsw_reverse_workspace_bytes': (c_i64, [c_i64, c_i64, c_int, c_int]),
    'nafp_hnsw_search_workspace_bytes': (c_i64, [c_i64, c_int, c_int]),
    'nafp_hnsw_search_layer': (c_int, [c_void_p, c_i64, c_int, c_void_p, c_void_p, c_i64, c_i64, c_int, c_int, c_void_p, c_i64, c_void_p,
                                       c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'nafp_hnsw_select_forward': (c_int, [c_void_p, c_i64, c_int, c_i64, c_i64, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                         c_void_p, c_i64, c_i64, c_void_p]),
    'nafp_hnsw_reverse_links': (c_int, [c_void_p, c_i64, c_int, c_i64, c_i64, c_void_p, c_int, c_int, c_void_p, c_void_p, c_i64, c_i64,
                                        c_void_p, c_i64, c_void_p]),
    'nafp_hnsw_search': (c_int, [c_void_p, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_int, c_void_p, c_i64, c_int,
                                 c_int, c_void_p, c_void_p, c_void_p, c_i64, c_void_p]),
    'nafp_minisearch_scores': (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_int, c_int, c_void_p, c_void_p]),
    'nafp_minisearch_ranks': (c_int, [c_void_p, c_i64, c_i64, c_int, c_int, c_int, c_void_p, c_void_p]),
    'nafp_lamb_step': (c_int, [c_void_p, c_int, c_float, c_float, c_float, c_float, c_float, c_i64,
                               c_void_p, c_i64, c_void_p]),
}


class OptTensor(ctypes.Structure):
    """nafp_opt_tensor (include/nafp.h)."""
    _fields_ = [('param', c_void_p), ('grad', c_void_p), ('m', c_void_p), ('v', c_void_p),
                ('numel', c_i64), ('var_len', c_i64)]


class Rect(ctypes.Structure):
    """nafp_rect (include/nafp.h): inclusive hole bounds."""
    _fields_ = [('f0', c_int), ('f1', c_int), ('t0', c_int), ('t1', c_int)]


# nafp_aug_row (include/nafp.h) as a numpy structured dtype: 64 bytes per row
AUG_ROW_DTYPE = [('ev_off', '<i8'), ('nz_off', '<i8'), ('nz2_off', '<i8'), ('ir_off', '<i8'), ('ev_valid', '<i4'),
                 ('nz_valid', '<i4'), ('nz2_valid', '<i4'), ('ir_len', '<i4'), ('snr_db', '<f4'), ('amp', '<f4'),
                 ('mix', '<i4'), ('reserved', '<i4')]
# nafp_aug_speed (include/nafp.h), one per row next to the nafp_aug_row table: 32 bytes
AUG_SPEED_DTYPE = [('file_off', '<i8'), ('n_in', '<i8'), ('out0', '<i8'), ('slot', '<i4'), ('reserved', '<i4')]


# nafp_resample_piece (include/nafp.h) as a numpy structured dtype: 56 bytes per piece
RESAMPLE_PIECE_DTYPE = [('raw_off', '<i8'), ('frame0', '<i8'), ('n_frames', '<i8'), ('n_in', '<i8'), ('out0', '<i8'),
                        ('out_off', '<i8'), ('n_out', '<i4'), ('channels', '<i4')]


# nafp_ingest_piece (include/nafp.h) as a numpy structured dtype: 64 bytes per piece; raw_off counts BYTES
INGEST_PIECE_DTYPE = [('raw_off', '<i8'), ('frame0', '<i8'), ('n_frames', '<i8'), ('n_in', '<i8'), ('out0', '<i8'),
                      ('out_off', '<i8'), ('n_out', '<i4'), ('channels', '<i4'), ('format', '<i4'), ('reserved', '<i4')]
# NAFP_INGEST_* format codes (include/nafp.h): name -> (code, bytes per sample)
INGEST_FORMATS = {'u8': (1, 1), 's16': (2, 2), 's24': (3, 3), 's32': (4, 4), 'f32': (5, 4), 'f64': (6, 8), 's8': (8, 1),
                  's16be': (18, 2), 's24be': (19, 3), 's32be': (20, 4), 'f32be': (21, 4), 'f64be': (22, 8)}      # NAFP_INGEST_BE = 16

# nafp_varispeed_piece (include/nafp.h) as a numpy structured dtype: 56 bytes per piece
VARISPEED_PIECE_DTYPE = [('src_off', '<i8'), ('frame0', '<i8'), ('n_frames', '<i8'), ('n_in', '<i8'), ('out0', '<i8'),
                         ('out_off', '<i8'), ('n_out', '<i4'), ('reserved', '<i4')]
VARISPEED_STEP_MIN, VARISPEED_STEP_MAX = 13421773, 20971520      # NAFP_VARISPEED_STEP_* (include/nafp.h): sigma 0.8 .. 1.25

# nafp_codec_piece (include/nafp.h) as a numpy structured dtype: 40 bytes per piece; raw_off counts BYTES, out_off int16
CODEC_PIECE_DTYPE = [('raw_off', '<i8'), ('n_blocks', '<i8'), ('out_off', '<i8'), ('codec', '<i4'), ('channels', '<i4'),
                     ('block_align', '<i4'), ('spb', '<i4')]
# NAFP_CODEC_* codes (include/nafp.h): the `format` name riff_scan_ex / aiff_scan / au_scan give such a file -> code
CODECS = {'alaw': 1, 'ulaw': 2, 'ima4': 3, 'ms4': 4, 'qtima4': 6}

# nafp_flac_info / nafp_flac_index_entry / nafp_flac_frame (include/nafp.h) as numpy structured dtypes: 72 / 32 / 40 bytes
FLAC_INFO_DTYPE = [('total_samples', '<i8'), ('audio_off', '<i8'), ('n_indexed', '<i8'), ('indexed_samples', '<i8'), ('rate', '<i4'),
                   ('channels', '<i4'), ('bps', '<i4'), ('min_block', '<i4'), ('max_block', '<i4'), ('refusal', '<i4'), ('md5', 'u1', (16,))]
FLAC_INDEX_DTYPE = [('offset', '<i8'), ('first_sample', '<i8'), ('n_bytes', '<i8'), ('block_size', '<i4'), ('reserved', '<i4')]
FLAC_FRAME_DTYPE = [('raw_off', '<i8'), ('scratch_off', '<i8'), ('n_bytes', '<i4'), ('block_size', '<i4'), ('channels', '<i4'),
                    ('bps', '<i4'), ('rate', '<i4'), ('reserved', '<i4')]


class NafpError(RuntimeError):
    pass


_lib = None


def load():
    """Load libnafp.so (once).  Raises NafpError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NafpError(
            f'{LIB_PATH} is missing: the HIP extension is not built. '
            'Run `python neural-audio-fp_amd/build.py` (or __graft_entry__.build()). '
            'There is no CPU fallback for this path.')
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)       # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.nafp_abi_version() != 1:
        raise NafpError('libnafp ABI version mismatch')
    _lib = lib
    return lib


def check(status, what=''):
    if status != 0:
        lib = load()
        msg = lib.nafp_status_string(status).decode()
        extra = ''
        if status == 3:
            extra = f' (hipError_t={lib.nafp_last_hip_error()})'
        raise NafpError(f'libnafp {what}: {msg}{extra}')


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else c_void_p(t.data_ptr())


def current_stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def require_cuda(t, name='tensor'):
    if not t.is_cuda:
        raise NafpError(f'{name} must live on the GPU (got {t.device}); this path has no CPU fallback')
    return t
