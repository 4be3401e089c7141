"""ctypes binding of include/he_amd.h (no compute happens in Python)."""
import collections
import ctypes
import os

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# HEAMD_LIBRARY points at another build of the same ABI (a deployment's install path, or an A/B kernel experiment:
# bench_tools/ab_variants.py)
_LIB_PATH = os.environ.get("HEAMD_LIBRARY") or os.path.join(_PKG, "lib", "libhe_amd.so")

U64P = ctypes.POINTER(ctypes.c_uint64)
vp = ctypes.c_void_p
HOST_CALLBACK = ctypes.CFUNCTYPE(None, ctypes.c_void_p)
c_u64 = ctypes.c_uint64
c_u32 = ctypes.c_uint32
c_size = ctypes.c_size_t


class Word(collections.namedtuple("Word", "bits suffix dtype")):
    """The word of a device slab: its bit count, the suffix of the C entries that take it and its torch dtype's name."""

    __slots__ = ()


WORD64 = Word(64, "", "int64")
WORD32 = Word(32, "_u32", "int32")  # packed [UInt32]: int32 tensors


def _word_of(word_bits):
    return WORD32 if word_bits == 32 else WORD64

STATUS_NAMES = {
    0: "ok", 1: "invalidDegree", 2: "invalidModulus", 3: "coprimeModuli", 4: "emptyModulus",
    5: "invalidNttModulus", 6: "invalidPolyContext", 7: "polyContextMismatch", 8: "invalidCiphertext",
    9: "incompatibleCiphertexts", 10: "incompatibleCiphertextAndPlaintext", 11: "missingRelinearizationKey",
    12: "unequalContexts", 13: "notEnoughPrimes", 14: "notInvertible", 15: "invalidEncryptionParameters",
    16: "invalidArgument", 17: "deviceError", 18: "unsupportedHeOperation", 19: "missingGaloisKey",
    20: "serializedBufferSizeMismatch", 21: "invalidCoefficientPacking", 22: "simdEncodingNotSupported",
    23: "invalidDatabaseSerializationVersion", 24: "invalidDatabaseSerializationPlaintextTag",
    25: "failedToConstructCuckooTable", 26: "invalidCuckooConfig", 27: "invalidHashBucketEntryValueSize",
    28: "invalidHashBucketSlotCount", 29: "cuckooTableNeedsExpansion", 30: "invalidSharding",
}


class HeError(RuntimeError):
    """Mirror of the reference's thrown HeError (HomomorphicEncryption/Error.swift:19-54)."""

    def __init__(self, code, detail=""):
        self.code = code
        self.name = STATUS_NAMES.get(code, "unknown")
        super().__init__(f"HeError.{self.name} ({code}) {detail}".strip())


# Every symbol include/he_amd.h declares: (name, restype, argtypes).  The 4-byte twin of an entry in _TWINNED is not spelled
# out: it has the name with WORD32's suffix and the same types.
SIGNATURES = [
    ("he_status_string", ctypes.c_char_p, [ctypes.c_int]),
    ("he_last_error_message", ctypes.c_char_p, []),
    ("he_version", ctypes.c_char_p, []),
    ("he_device_count", ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    ("he_words_copy_device", ctypes.c_int, [vp, vp, c_size, ctypes.c_int, vp]),
    ("he_get_device", ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    ("he_set_device", ctypes.c_int, [ctypes.c_int]),
    ("he_set_scratch_cache", ctypes.c_int, [c_u64]),
    ("he_device_trim_scratch", ctypes.c_int, [c_u64]),
    ("he_scratch_cached_bytes", ctypes.c_int, [ctypes.POINTER(c_u64)]),
    ("he_shard_bounds", ctypes.c_int, [c_size, c_u32, c_u32, ctypes.POINTER(c_size), ctypes.POINTER(c_size)]),
    ("he_device_group_create", ctypes.c_int, [ctypes.POINTER(ctypes.c_int), c_u32, c_u32, c_u32, c_u64,
                                              ctypes.POINTER(c_u64), c_u32, ctypes.POINTER(vp)]),
    ("he_device_group_destroy", None, [vp]),
    ("he_device_group_size", c_u32, [vp]),
    ("he_device_group_device", ctypes.c_int, [vp, c_u32, ctypes.POINTER(ctypes.c_int)]),
    ("he_device_group_context", vp, [vp, c_u32]),
    ("he_device_group_stream", vp, [vp, c_u32]),
    ("he_device_group_synchronize", ctypes.c_int, [vp]),
    ("he_ntt_forward_group", ctypes.c_int, [vp, c_u32, ctypes.POINTER(vp), c_size]),
    ("he_ntt_inverse_group", ctypes.c_int, [vp, c_u32, ctypes.POINTER(vp), c_size]),
    ("he_pir_dim0_columns_group", ctypes.c_int, [vp, vp, c_size, ctypes.POINTER(vp), ctypes.POINTER(vp), c_size, vp, vp]),
    ("he_pir_compute_response_chunk_group", ctypes.c_int, [vp, ctypes.POINTER(c_u32), c_u32, vp, vp, c_size,
                                                           ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp, vp]),
    ("he_pir_compute_response_group", ctypes.c_int, [vp, ctypes.POINTER(c_u32), c_u32, vp, vp, c_size, ctypes.POINTER(vp),
                                                     ctypes.POINTER(vp), c_size, vp, vp, vp]),
    ("he_pir_remaining_dimensions_chunks_device", ctypes.c_int, [vp, ctypes.POINTER(c_u32), c_u32, c_size, vp, vp, c_size, vp,
                                                                 vp, vp]),
    ("he_device_malloc", ctypes.c_int, [ctypes.POINTER(vp), c_size]),
    ("he_device_free", ctypes.c_int, [vp]),
    ("he_host_malloc", ctypes.c_int, [ctypes.POINTER(vp), c_size]),
    ("he_host_free", ctypes.c_int, [vp]),
    ("he_memcpy_h2d", ctypes.c_int, [vp, vp, c_size, vp]),
    ("he_memcpy_d2h", ctypes.c_int, [vp, vp, c_size, vp]),
    ("he_stream_synchronize", ctypes.c_int, [vp]),
    ("he_stream_create", ctypes.c_int, [ctypes.POINTER(vp)]),
    ("he_stream_destroy", ctypes.c_int, [vp]),
    ("he_event_create", ctypes.c_int, [ctypes.POINTER(vp)]),
    ("he_event_destroy", ctypes.c_int, [vp]),
    ("he_event_record", ctypes.c_int, [vp, vp]),
    ("he_event_synchronize", ctypes.c_int, [vp]),
    ("he_event_query", ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_int)]),
    ("he_stream_wait_event", ctypes.c_int, [vp, vp]),
    ("he_stream_add_callback", ctypes.c_int, [vp, HOST_CALLBACK, vp]),
    ("he_poly_context_create", ctypes.c_int, [c_u32, U64P, c_u32, ctypes.POINTER(vp)]),
    ("he_poly_context_destroy", None, [vp]),
    ("he_poly_context_degree", c_u32, [vp]),
    ("he_poly_context_moduli_count", c_u32, [vp]),
    ("he_poly_context_moduli", ctypes.c_int, [vp, U64P]),
    ("he_poly_context_max_lazy_product_accumulation_count", c_u64, [vp]),
    ("he_poly_context_q_remainder", ctypes.c_int, [vp, c_u64, U64P]),
    ("he_generate_primes", ctypes.c_int, [ctypes.POINTER(ctypes.c_int32), c_u32, ctypes.c_int, c_u32, U64P]),
    ("he_ntt_forward", ctypes.c_int, [vp, U64P, c_size]),
    ("he_ntt_inverse", ctypes.c_int, [vp, U64P, c_size]),
    ("he_ntt_forward_device", ctypes.c_int, [vp, vp, c_size, vp]),
    ("he_ntt_inverse_device", ctypes.c_int, [vp, vp, c_size, vp]),
    ("he_ntt_forward_rows_device", ctypes.c_int, [vp, c_u64, vp, c_size, vp]),
    ("he_ntt_inverse_rows_device", ctypes.c_int, [vp, c_u64, vp, c_size, vp]),
    ("he_poly_add_device", ctypes.c_int, [vp, vp, vp, c_size, vp]),
    ("he_poly_sub_device", ctypes.c_int, [vp, vp, vp, c_size, vp]),
    ("he_poly_neg_device", ctypes.c_int, [vp, vp, c_size, vp]),
    ("he_poly_mul_device", ctypes.c_int, [vp, vp, vp, c_size, vp]),
    ("he_poly_mul_scalar_device", ctypes.c_int, [vp, vp, U64P, c_size, vp]),
    ("he_poly_divide_and_round_q_last_device", ctypes.c_int, [vp, vp, vp, c_size, vp]),
    ("he_poly_divide_and_round_q_last", ctypes.c_int, [vp, U64P, U64P, c_size]),
    ("he_poly_adding_lazy_product_device", ctypes.c_int, [vp, vp, vp, vp, vp]),
    ("he_poly_reduce_accumulator_device", ctypes.c_int, [vp, vp, vp, vp]),
    ("he_poly_apply_galois_device", ctypes.c_int, [vp, vp, vp, c_size, c_u64, ctypes.c_int, vp]),
    ("he_poly_random_from_seeds_device", ctypes.c_int, [vp, vp, c_size, vp, vp]),
    ("he_poly_mul_scalar_device_u32", ctypes.c_int, [vp, vp, ctypes.POINTER(ctypes.c_uint32), c_size, vp]),
    ("he_words_widen_u32_device", ctypes.c_int, [vp, vp, c_size, vp]),
    ("he_words_narrow_u64_device", ctypes.c_int, [vp, vp, c_size, vp]),
    ("he_poly_serialization_byte_count", c_size, [vp, ctypes.c_int]),
    ("he_poly_serialize_device", ctypes.c_int, [vp, vp, c_size, ctypes.c_int, vp, vp]),
    ("he_poly_deserialize_device", ctypes.c_int, [vp, vp, c_size, c_size, ctypes.c_int, vp, vp]),
    ("he_bfv_skip_lsbs_for_decryption", ctypes.c_int, [c_u32, c_u64, c_u64, c_u32, ctypes.POINTER(ctypes.c_int)]),
    ("he_ciphertexts_serialization_byte_count", c_size, [vp, c_u32, ctypes.POINTER(ctypes.c_int)]),
    ("he_ciphertexts_wire_plan", ctypes.c_int,
     [ctypes.c_int, c_u32, vp, c_u32, ctypes.POINTER(ctypes.c_int), c_size, c_u64, c_u64, ctypes.POINTER(c_u32),
      ctypes.POINTER(c_size), ctypes.POINTER(c_size), ctypes.POINTER(c_u32)]),
    ("he_ciphertexts_serialize_device", ctypes.c_int,
     [vp, vp, c_size, c_u32, ctypes.POINTER(ctypes.c_int), vp, c_size, vp]),
    ("he_ciphertexts_deserialize_device", ctypes.c_int,
     [vp, vp, c_size, c_size, c_u32, ctypes.POINTER(ctypes.c_int), vp, vp, vp]),
    ("he_ciphertexts_deserialize_seeded_device", ctypes.c_int, [vp, vp, c_size, vp, c_size, ctypes.c_int, vp, vp]),
    ("he_poly_multiply_power_of_x_device", ctypes.c_int, [vp, vp, vp, c_size, ctypes.c_int64, vp]),
    ("he_bfv_context_create", ctypes.c_int, [c_u32, c_u64, U64P, c_u32, ctypes.POINTER(vp)]),
    ("he_bfv_context_destroy", None, [vp]),
    ("he_bfv_ciphertext_moduli_count", c_u32, [vp]),
    ("he_bfv_ciphertext_context", vp, [vp, c_u32]),
    ("he_bfv_key_switching_context", vp, [vp, c_u32]),
    ("he_bfv_qbsk_context", vp, [vp, c_u32]),
    ("he_rns_lift_q_to_qbsk_device", ctypes.c_int, [vp, c_u32, vp, vp, c_size, vp]),
    ("he_rns_floor_qbsk_to_q_device", ctypes.c_int, [vp, c_u32, vp, vp, c_size, vp]),
    ("he_bfv_mul_workspace_bytes", c_size, [vp, c_u32, c_size]),
    ("he_bfv_relinearize_workspace_bytes", c_size, [vp, c_u32, c_size]),
    ("he_bfv_inner_product_workspace_bytes", c_size, [vp, c_u32, c_size]),
    ("he_bfv_mul_device", ctypes.c_int, [vp, c_u32, vp, vp, vp, c_size, vp, c_size, vp]),
    ("he_bfv_relinearize_device", ctypes.c_int, [vp, c_u32, vp, vp, vp, c_size, vp, c_size, vp]),
    ("he_bfv_mod_switch_down_device", ctypes.c_int, [vp, c_u32, c_u32, vp, vp, c_size, vp]),
    ("he_bfv_mod_switch_down_to_single_device", ctypes.c_int, [vp, c_u32, c_u32, vp, vp, c_size, vp]),
    ("he_bfv_mul_plain_device", ctypes.c_int, [vp, c_u32, c_u32, vp, vp, c_size, vp]),
    ("he_bfv_add_plain_device", ctypes.c_int, [vp, c_u32, c_u32, vp, vp, c_size, vp]),
    ("he_bfv_sub_plain_device", ctypes.c_int, [vp, c_u32, c_u32, vp, vp, c_size, vp]),
    ("he_bfv_inner_product_plain_device", ctypes.c_int,
     [vp, c_u32, c_u32, vp, vp, ctypes.POINTER(ctypes.c_uint8), c_size, c_size, vp, vp]),
    ("he_bfv_inner_product_plain_resident_device", ctypes.c_int,
     [vp, c_u32, c_u32, vp, vp, vp, c_size, c_size, vp, vp]),
    ("he_bfv_inner_product_device", ctypes.c_int, [vp, c_u32, vp, vp, c_size, vp, vp, c_size, vp]),
    ("he_bfv_inner_product_shared_device", ctypes.c_int, [vp, c_u32, vp, vp, c_size, c_size, vp, vp]),
    ("he_bfv_packed_plaintext_words", c_size, [vp, c_u32]),
    ("he_bfv_pack_plaintexts_device", ctypes.c_int, [vp, c_u32, vp, c_size, vp, vp]),
    ("he_bfv_inner_product_plain_packed_device", ctypes.c_int, [vp, c_u32, c_u32, vp, vp, vp, c_size, c_size, vp, vp]),
    ("he_pir_dim0_columns_packed_device", ctypes.c_int, [vp, vp, c_size, vp, vp, c_size, vp, vp]),
    ("he_pir_compute_response_to_query_device", ctypes.c_int,
     [vp, ctypes.POINTER(c_u32), c_u32, vp, c_size, c_size, U64P, ctypes.POINTER(vp), c_size, vp, ctypes.POINTER(vp),
      ctypes.POINTER(vp), c_size, c_size, vp, vp]),
    ("he_pir_compute_response_packed_device", ctypes.c_int,
     [vp, ctypes.POINTER(c_u32), c_u32, vp, vp, c_size, vp, vp, c_size, vp, vp, vp]),
    ("he_galois_element_swapping_rows", ctypes.c_int, [c_u64, U64P]),
    ("he_galois_element_rotating_columns", ctypes.c_int, [ctypes.c_int64, c_u64, U64P]),
    ("he_bfv_apply_galois_workspace_bytes", c_size, [vp, c_u32, c_size]),
    ("he_bfv_apply_galois_device", ctypes.c_int, [vp, c_u32, vp, c_u64, vp, vp, c_size, vp, c_size, vp]),
    ("he_rns_scale_and_round_device", ctypes.c_int, [vp, c_u32, vp, c_u64, vp, c_size, vp]),
    ("he_bfv_plaintext_to_eval_device", ctypes.c_int, [vp, c_u32, vp, vp, c_size, vp]),
    ("he_bfv_plaintext_to_coeff_device", ctypes.c_int, [vp, c_u32, vp, vp, c_size, vp]),
    # decryption of resident ciphertexts: the slab word is an argument (word_bits), so these have no 4-byte twins
    ("he_bfv_decrypt_workspace_bytes", c_size, [vp, c_u32, c_u32, c_u32, ctypes.c_int, c_size]),
    ("he_bfv_secret_dot_product_device", ctypes.c_int, [vp, c_u32, c_u32, c_u32, ctypes.c_int, vp, vp, vp, c_size, vp, c_size,
                                                        vp]),
    ("he_bfv_decrypt_device", ctypes.c_int, [vp, c_u32, c_u32, c_u32, ctypes.c_int, vp, vp, c_u64, vp, c_size, vp, c_size, vp]),
    ("he_bfv_noise_norm_device", ctypes.c_int, [vp, c_u32, c_u32, c_u32, ctypes.c_int, vp, vp, vp, c_size, vp, c_size, vp]),
    ("he_bfv_is_transparent_device", ctypes.c_int, [vp, c_u32, c_u32, c_u32, vp, vp, c_size, vp]),
    ("he_bfv_noise_norm_limbs", c_u32, [vp, c_u32]),
    ("he_bfv_noise_budget_from_norm", ctypes.c_int, [vp, c_u32, c_u32, U64P, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    # secret keys, encryption, evaluation keys from caller-supplied seeds: word_bits is an argument here too
    ("he_bfv_encrypt_workspace_bytes", c_size, [vp, c_u32, ctypes.c_int, c_u32, ctypes.c_int, c_size]),
    ("he_bfv_generate_secret_key_device", ctypes.c_int, [vp, c_u32, vp, vp, c_size, vp, c_size, vp]),
    ("he_bfv_encrypt_zero_device", ctypes.c_int, [vp, c_u32, c_u32, ctypes.c_int, vp, vp, vp, vp, c_size, vp, c_size, vp]),
    ("he_bfv_encrypt_device", ctypes.c_int, [vp, c_u32, c_u32, vp, vp, vp, vp, vp, c_size, vp, c_size, vp]),
    ("he_bfv_generate_key_switch_keys_device", ctypes.c_int, [vp, c_u32, vp, vp, vp, vp, vp, c_size, vp, c_size, vp]),
    ("he_bfv_generate_relinearization_key_device", ctypes.c_int, [vp, c_u32, vp, vp, vp, vp, vp, c_size, vp]),
    ("he_bfv_generate_galois_keys_device", ctypes.c_int, [vp, c_u32, vp, U64P, c_size, vp, vp, vp, vp, c_size, vp]),
    ("he_poly_random_ternary_from_seeds_device", ctypes.c_int, [vp, c_u32, vp, c_size, vp, vp]),
    ("he_poly_random_centered_binomial_from_seeds_device", ctypes.c_int, [vp, c_u32, vp, c_size, vp, vp]),
    ("he_pir_compute_response_chunk_device", ctypes.c_int,
     [vp, ctypes.POINTER(c_u32), c_u32, vp, vp, c_size, vp, ctypes.POINTER(ctypes.c_uint8), vp, vp, vp]),
    ("he_pir_dim0_columns_device", ctypes.c_int, [vp, vp, c_size, vp, vp, c_size, vp, vp]),
    ("he_pir_remaining_dimensions_device", ctypes.c_int,
     [vp, ctypes.POINTER(c_u32), c_u32, vp, vp, c_size, vp, vp, vp]),
    ("he_pir_compute_response_device", ctypes.c_int,
     [vp, ctypes.POINTER(c_u32), c_u32, vp, vp, c_size, vp, vp, c_size, vp, vp, vp]),
    ("he_pir_compute_response_queries_device", ctypes.c_int,
     [vp, ctypes.POINTER(c_u32), c_u32, c_size, vp, vp, c_size, vp, vp, c_size, ctypes.POINTER(vp), vp, vp]),
    ("he_pir_expand_batch_device", ctypes.c_int,
     [vp, vp, c_size, c_size, c_size, U64P, ctypes.POINTER(vp), c_size, vp, vp]),
    ("he_bfv_apply_galois_grouped_device", ctypes.c_int,
     [vp, c_u32, vp, c_u64, ctypes.POINTER(vp), c_size, c_size, vp, vp, c_size, vp]),
    ("he_pir_expand_device", ctypes.c_int,
     [vp, vp, c_size, c_size, U64P, ctypes.POINTER(vp), c_size, vp, vp]),
    ("he_pir_database_shape", ctypes.c_int,
     [vp, ctypes.POINTER(c_u32), c_u32, c_size, c_size, ctypes.c_int, ctypes.POINTER(c_size), ctypes.POINTER(c_size),
      ctypes.POINTER(c_size), ctypes.POINTER(c_size), ctypes.POINTER(c_size)]),
    ("he_pir_process_database_device", ctypes.c_int,
     [vp, ctypes.POINTER(c_u32), c_u32, vp, U64P, c_size, c_size, ctypes.c_int, vp, vp, vp]),
    ("he_pir_client_plan", ctypes.c_int,
     [vp, ctypes.POINTER(c_u32), c_u32, c_size, c_size, ctypes.c_int, c_size] + [ctypes.POINTER(c_size)] * 6),
    ("he_pir_evaluation_key_elements", ctypes.c_int, [c_u32, c_size, ctypes.c_int, U64P, c_size, ctypes.POINTER(c_size)]),
    ("he_pir_generate_query_workspace_bytes", c_size,
     [vp, c_u32, ctypes.POINTER(c_u32), c_u32, c_size, c_size, ctypes.c_int, c_size, c_size]),
    ("he_pir_generate_query_device", ctypes.c_int,
     [vp, c_u32, ctypes.POINTER(c_u32), c_u32, c_size, c_size, ctypes.c_int, c_size, vp, c_size, vp, vp, vp, vp, vp, vp,
      c_size, vp]),
    ("he_pir_decrypt_response_workspace_bytes", c_size,
     [vp, c_u32, ctypes.POINTER(c_u32), c_u32, c_size, c_size, ctypes.c_int, c_size, c_u32, c_size]),
    ("he_pir_decrypt_response_device", ctypes.c_int,
     [vp, c_u32, ctypes.POINTER(c_u32), c_u32, c_size, c_size, ctypes.c_int, c_size, c_u32, vp, vp, c_size, vp, vp, vp, vp,
      c_size, vp]),
    ("he_pir_database_file_scan", ctypes.c_int,
     [vp, vp, c_size, vp, c_size, ctypes.POINTER(c_size), ctypes.POINTER(c_size), ctypes.POINTER(c_size)]),
    ("he_pir_database_file_byte_count", ctypes.c_int, [vp, vp, c_size, ctypes.POINTER(c_size)]),
    ("he_pir_database_file_header", ctypes.c_int, [c_size, vp]),
    ("he_pir_database_load_device", ctypes.c_int, [vp, vp, c_size, vp, c_size, vp, vp, vp]),
    ("he_pir_database_save_device", ctypes.c_int, [vp, vp, vp, c_size, vp, c_size, vp, vp]),
    ("he_keyword_pir_hash_keywords_device", ctypes.c_int, [vp, vp, c_size, vp, vp]),
    ("he_keyword_pir_hash_indices_device", ctypes.c_int, [vp, c_size, c_u64, c_u32, vp, vp]),
    ("he_keyword_pir_shard_indices_device", ctypes.c_int, [vp, c_size, c_u64, c_u64, vp, vp]),
    ("he_keyword_pir_config_validate", ctypes.c_int, [vp]),
    ("he_keyword_pir_bucket_count", ctypes.c_int, [vp, U64P, c_size, ctypes.POINTER(c_size)]),
    ("he_keyword_pir_cuckoo_place", ctypes.c_int,
     [vp, U64P, ctypes.POINTER(c_u32), U64P, c_size, c_size, c_u64, ctypes.POINTER(c_u32), ctypes.POINTER(c_u32),
      ctypes.POINTER(c_size), ctypes.POINTER(c_size), ctypes.POINTER(c_size)]),
    ("he_keyword_pir_serialize_buckets_device", ctypes.c_int, [vp, vp, vp, vp, vp, c_size, c_size, c_size, vp, vp, vp]),
    ("he_keyword_pir_table_create_device", ctypes.c_int, [vp, vp, U64P, vp, U64P, c_size, c_u64, ctypes.POINTER(vp), vp]),
    ("he_keyword_pir_table_destroy", None, [vp]),
    ("he_keyword_pir_table_bucket_count", c_size, [vp]),
    ("he_keyword_pir_table_buckets_per_table", c_size, [vp]),
    ("he_keyword_pir_table_table_count", c_size, [vp]),
    ("he_keyword_pir_table_largest_bucket_size", c_size, [vp]),
    ("he_keyword_pir_table_entry_count", c_size, [vp]),
    ("he_keyword_pir_table_duplicates_dropped", c_size, [vp]),
    ("he_keyword_pir_table_expansion_count", c_size, [vp]),
    ("he_keyword_pir_table_load_factor", ctypes.c_float, [vp]),
    ("he_keyword_pir_table_entries_device", ctypes.c_int, [vp, vp, c_size, vp, vp]),
    ("he_keyword_pir_process_database_device", ctypes.c_int, [vp, vp, vp, ctypes.POINTER(c_u32), c_u32, c_size, vp, vp, vp]),
    ("he_keyword_client_plan", ctypes.c_int,
     [vp, ctypes.POINTER(c_u32), c_u32, c_size, c_size, c_u32] + [ctypes.POINTER(c_size)] * 6 +
     [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(c_size), ctypes.POINTER(c_size)]),
    ("he_keyword_client_generate_query_workspace_bytes", c_size,
     [vp, c_u32, ctypes.POINTER(c_u32), c_u32, c_size, c_size, c_u32, c_size]),
    ("he_keyword_client_generate_query_device", ctypes.c_int,
     [vp, c_u32, ctypes.POINTER(c_u32), c_u32, c_size, c_size, c_u32, vp, vp, c_size, vp, vp, vp, vp, vp, vp, c_size, vp]),
    ("he_keyword_client_find_in_buckets_workspace_bytes", c_size, [c_size, c_u32, c_size]),
    ("he_keyword_client_find_in_buckets_device", ctypes.c_int,
     [vp, vp, c_size, c_u32, c_size, ctypes.c_int, vp, vp, vp, vp, c_size, vp]),
    ("he_keyword_client_decrypt_response_workspace_bytes", c_size,
     [vp, c_u32, ctypes.POINTER(c_u32), c_u32, c_size, c_size, c_u32, c_u32, c_size]),
    ("he_keyword_client_decrypt_response_device", ctypes.c_int,
     [vp, c_u32, ctypes.POINTER(c_u32), c_u32, c_size, c_size, c_u32, c_u32, vp, vp, vp, vp, c_size, vp, vp, vp, vp, vp,
      c_size, vp]),
    ("he_keyword_client_count_entries_workspace_bytes", c_size,
     [vp, c_u32, ctypes.POINTER(c_u32), c_u32, c_size, c_size, c_u32, c_u32, c_size]),
    ("he_keyword_client_count_entries_device", ctypes.c_int,
     [vp, c_u32, ctypes.POINTER(c_u32), c_u32, c_size, c_size, c_u32, c_u32, vp, c_size, vp, vp, vp, c_size, vp]),
    ("he_keyword_client_count_bucket_entries_device", ctypes.c_int, [vp, c_size, c_size, c_size, vp, vp]),
    ("he_keyword_sharding_shard_count", ctypes.c_int, [vp, c_size, ctypes.POINTER(c_size)]),
    ("he_keyword_database_partition_device", ctypes.c_int,
     [vp, vp, c_size, vp, vp, c_size, c_size, vp, c_size, vp, vp, vp, vp, vp, vp, vp, vp]),
    ("he_keyword_database_partition_plan", ctypes.c_int,
     [c_size, c_size, c_size, c_size, ctypes.POINTER(c_u32), ctypes.POINTER(c_size), ctypes.POINTER(c_u32),
      ctypes.POINTER(c_size), ctypes.POINTER(c_u32), ctypes.POINTER(c_u32)]),
    ("he_keyword_database_create_device", ctypes.c_int,
     [vp, vp, U64P, vp, U64P, c_size, c_size, c_u64, c_u64, ctypes.POINTER(vp), vp]),
    ("he_keyword_database_destroy", None, [vp]),
    ("he_keyword_database_shard_count", c_size, [vp]),
    ("he_keyword_database_shard_row_count", c_size, [vp, c_size]),
    ("he_keyword_database_shard_table", vp, [vp, c_size]),
    ("he_keyword_database_shard_values", vp, [vp, c_size]),
    ("he_keyword_database_order", ctypes.c_int, [vp, ctypes.POINTER(c_u32)]),
    ("he_simple_pir_shape", ctypes.c_int,
     [c_u32, c_u32, c_u32, c_u32, c_size, c_size, ctypes.POINTER(c_size), ctypes.POINTER(c_size), ctypes.POINTER(c_size),
      ctypes.POINTER(c_size), ctypes.POINTER(c_size), ctypes.POINTER(c_size), ctypes.POINTER(c_u64), ctypes.POINTER(c_u32)]),
    ("he_simple_pir_context_create", ctypes.c_int, [c_u32, c_u32, c_u32, c_u32, c_size, c_size, ctypes.POINTER(vp)]),
    ("he_simple_pir_context_destroy", None, [vp]),
    ("he_simple_pir_process_database_device", ctypes.c_int, [vp, vp, vp, vp, vp, vp]),
    ("he_simple_pir_pack_database_device", ctypes.c_int, [c_u32, vp, vp, c_size, vp]),
    ("he_simple_pir_unpack_database_device", ctypes.c_int, [c_u32, vp, vp, c_size, vp]),
    ("he_simple_pir_compute_response_device", ctypes.c_int, [c_u32, c_u32, vp, c_size, c_size, vp, c_size, vp, vp]),
    ("he_simple_pir_compute_response_batch_device", ctypes.c_int, [c_u32, c_u32, vp, c_size, c_size, vp, c_size, vp, vp]),
    ("he_simple_pir_batch_response_plan", ctypes.c_int,
     [c_u32, c_u32, c_u32, c_size, c_size, ctypes.POINTER(c_u32), ctypes.POINTER(c_u32), ctypes.POINTER(c_u32),
      ctypes.POINTER(c_u32), ctypes.POINTER(c_size), ctypes.POINTER(c_size)]),
    ("he_simple_pir_client_plan", ctypes.c_int,
     [c_u32, c_u32, c_u32, c_u32, c_size, c_size, ctypes.c_int, c_size, ctypes.POINTER(c_size), ctypes.POINTER(c_size),
      ctypes.POINTER(c_size), ctypes.POINTER(c_u32), ctypes.POINTER(c_u32), ctypes.POINTER(c_u64), ctypes.POINTER(c_size),
      ctypes.POINTER(c_size), ctypes.POINTER(c_size), ctypes.POINTER(c_size), ctypes.POINTER(c_size), ctypes.POINTER(c_size),
      ctypes.POINTER(c_size)]),
    ("he_simple_pir_client_workspace_bytes", c_size, [vp, ctypes.c_int, ctypes.c_int, c_size]),
    ("he_simple_pir_a_polynomials_device", ctypes.c_int, [vp, c_u32, vp, vp, vp, c_size, vp]),
    ("he_simple_pir_encrypt_zero_device", ctypes.c_int, [vp, c_u32, ctypes.c_int, vp, vp, vp, vp, c_size, vp, c_size, vp]),
    ("he_simple_pir_secret_times_hint_device", ctypes.c_int, [vp, c_u32, vp, c_size, vp, c_size, vp, vp, c_size, vp]),
    ("he_simple_pir_precompute_queries_device", ctypes.c_int,
     [vp, c_u32, ctypes.c_int, vp, vp, vp, vp, vp, vp, c_size, vp, c_size, vp]),
    ("he_simple_pir_add_indices_device", ctypes.c_int, [vp, c_u32, vp, vp, vp, c_size, vp]),
    ("he_simple_pir_decrypt_responses_device", ctypes.c_int, [vp, c_u32, vp, vp, vp, vp, vp, c_size, vp, c_size, vp]),
    ("he_simple_pir_shard_plan", ctypes.c_int,
     [U64P, c_size, c_size, c_size, c_u64, ctypes.POINTER(c_u64), ctypes.POINTER(c_u64), ctypes.POINTER(c_u64),
      ctypes.POINTER(c_u32), ctypes.POINTER(c_u32), ctypes.POINTER(c_size), ctypes.POINTER(c_size), ctypes.POINTER(c_size)]),
    ("he_simple_pir_shard_map_device", ctypes.c_int, [vp, vp, c_size, c_size, c_size, c_u64, vp, vp, vp, vp, vp, vp, vp]),
    ("he_simple_pir_shard_scatter_device", ctypes.c_int, [vp, c_u64, vp, c_size, c_size, c_u64, vp, vp, vp, vp]),
    ("he_simple_pir_shard_query_indices_device", ctypes.c_int,
     [vp, c_size, c_size, c_size, c_u64, c_u64, c_u64, vp, vp, vp, vp, vp, vp]),
    ("he_simple_pir_shard_assemble_device", ctypes.c_int,
     [vp, vp, vp, c_size, vp, c_size, c_size, c_size, c_u64, c_u64, c_u64, vp, vp, vp, vp, vp, vp, vp]),
    ("he_pnns_context_create", ctypes.c_int, [vp, ctypes.POINTER(vp)]),
    ("he_pnns_context_destroy", None, [vp]),
    ("he_pnns_matrix_shape", ctypes.c_int,
     [vp, c_size, c_size, ctypes.c_int, c_u32, ctypes.POINTER(c_size), ctypes.POINTER(c_u32), ctypes.POINTER(c_u32)]),
    ("he_pnns_quantize_rows_device", ctypes.c_int, [vp, c_size, c_size, ctypes.c_float, vp, vp]),
    ("he_pnns_diagonal_matrix_device", ctypes.c_int, [vp, vp, c_size, c_size, c_u32, ctypes.c_int, c_u32, vp, vp, vp]),
    ("he_pnns_mul_transpose_device", ctypes.c_int, [vp, vp, c_size, c_size, c_size, c_u32, vp, c_size, vp, vp, vp]),
    ("he_pnns_compute_response_device", ctypes.c_int, [vp, vp, c_size, c_size, c_size, c_u32, vp, c_size, vp, vp, vp]),
    ("he_pnns_query_matrix_shape", ctypes.c_int, [vp, c_size, c_size, c_size, vp, vp, vp]),
    ("he_pnns_mul_transpose_matrix_device", ctypes.c_int,
     [vp, vp, c_size, c_size, c_size, c_u32, vp, c_size, c_size, vp, c_size, vp, vp, vp]),
    ("he_pnns_compute_response_matrix_device", ctypes.c_int,
     [vp, vp, c_size, c_size, c_size, c_u32, vp, c_size, c_size, vp, c_size, vp, vp, vp]),
    ("he_pnns_simd_encode_device", ctypes.c_int, [vp, c_u32, vp, c_size, vp, vp, vp]),
    ("he_pnns_simd_decode_device", ctypes.c_int, [vp, c_u32, vp, c_size, vp, vp]),
    ("he_pnns_pack_dense_rows_device", ctypes.c_int, [vp, c_u32, vp, c_size, c_size, ctypes.c_int, vp, vp, vp]),
    ("he_pnns_unpack_device", ctypes.c_int, [vp, c_u32, ctypes.c_int, vp, c_size, c_size, vp, vp]),
    ("he_pnns_generate_query_workspace_bytes", c_size, [vp, c_size, c_u32, c_size, c_size]),
    ("he_pnns_generate_query_device", ctypes.c_int,
     [vp, c_size, c_u32, vp, c_size, c_size, ctypes.c_float, vp, vp, vp, vp, vp, vp, c_size, vp]),
    ("he_pnns_decrypt_response_workspace_bytes", c_size, [vp, c_size, c_u32, c_u32, c_size, c_size]),
    ("he_pnns_decrypt_response_device", ctypes.c_int,
     [vp, c_size, c_u32, c_u32, vp, vp, c_size, c_size, ctypes.c_float, vp, vp, c_size, vp]),
    # diagnostics / test hooks
    ("he_poly_context_create_host_only", ctypes.c_int, [c_u32, U64P, c_u32, ctypes.POINTER(vp)]),
    ("he_poly_context_copy_ntt_tables", ctypes.c_int, [vp, c_u32, U64P, U64P, U64P, U64P, U64P, U64P]),
    ("he_ntt_device_variant", ctypes.c_int, [vp, vp, c_size, ctypes.c_int, ctypes.c_int, vp]),
    ("he_bfv_context_create_host_only", ctypes.c_int, [c_u32, c_u64, U64P, c_u32, ctypes.POINTER(vp)]),
    ("he_bfv_context_create_u32_host_only", ctypes.c_int, [c_u32, c_u64, U64P, c_u32, ctypes.POINTER(vp)]),
    ("he_bfv_copy_bsk_moduli", ctypes.c_int, [vp, U64P]),
]
_TWINNED = (
    "he_ntt_forward_device", "he_ntt_inverse_device", "he_poly_add_device", "he_poly_sub_device", "he_poly_neg_device",
    "he_poly_mul_device", "he_poly_divide_and_round_q_last_device", "he_poly_serialize_device",
    "he_poly_deserialize_device", "he_poly_random_from_seeds_device", "he_ciphertexts_serialize_device",
    "he_ciphertexts_deserialize_device", "he_ciphertexts_deserialize_seeded_device", "he_bfv_context_create",
    "he_rns_lift_q_to_qbsk_device", "he_rns_floor_qbsk_to_q_device", "he_rns_scale_and_round_device",
    "he_bfv_mul_device", "he_bfv_relinearize_device", "he_bfv_apply_galois_device", "he_bfv_mod_switch_down_device",
    "he_bfv_mul_plain_device", "he_bfv_add_plain_device", "he_bfv_sub_plain_device",
    "he_bfv_inner_product_plain_resident_device", "he_bfv_inner_product_device", "he_bfv_inner_product_shared_device",
    "he_pir_compute_response_device", "he_pir_compute_response_queries_device",
    "he_pir_compute_response_to_query_device", "he_bfv_plaintext_to_eval_device", "he_bfv_plaintext_to_coeff_device",
    "he_pir_process_database_device", "he_pir_database_load_device", "he_pir_database_save_device",
    "he_simple_pir_process_database_device", "he_simple_pir_pack_database_device",
    "he_simple_pir_unpack_database_device", "he_simple_pir_compute_response_device",
    "he_simple_pir_compute_response_batch_device", "he_pnns_context_create", "he_pnns_diagonal_matrix_device",
    "he_pnns_mul_transpose_device", "he_pnns_compute_response_device", "he_pnns_mul_transpose_matrix_device",
    "he_pnns_compute_response_matrix_device",
)
_rows = {name: (restype, argtypes) for name, restype, argtypes in SIGNATURES}
SIGNATURES += [(name + WORD32.suffix,) + _rows[name] for name in _TWINNED]
del _rows

_lib = None


def library_path():
    return _LIB_PATH


def load_library():
    """Loads libhe_amd.so.  Fails loudly when it has not been built -- there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise ImportError(
                f"{_LIB_PATH} is missing: build the HIP extension first "
                "(python swift-homomorphic-encryption_amd/build.py, or __graft_entry__.build()).")
        try:
            # PyTorch ships its own libamdhip64.so.7 / libhsa-runtime64.so.1.  Import it first so that libhe_amd.so
            # binds to the SAME HIP runtime instance as the tensors it is handed (two runtimes in one process do not
            # see each other's devices).  Without PyTorch the library uses the system ROCm runtime.
            import torch  # noqa: F401
        except ImportError:  # pragma: no cover
            pass
        lib = ctypes.CDLL(_LIB_PATH)
        for name, restype, argtypes in SIGNATURES:
            fn = getattr(lib, name)  # AttributeError = header and library disagree
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = lib
    return _lib


def _check(code):
    if code != 0:
        detail = load_library().he_last_error_message().decode(errors="replace")
        raise HeError(code, detail)


def version():
    return load_library().he_version().decode()


def device_count():
    n = ctypes.c_int(0)
    _check(load_library().he_device_count(ctypes.byref(n)))
    return n.value


def current_device():
    n = ctypes.c_int(0)
    _check(load_library().he_get_device(ctypes.byref(n)))
    return n.value


def set_device(device):
    _check(load_library().he_set_device(device))


def set_scratch_cache(nbytes=2**64 - 1):
    """Let the library's scratch pool of the current device keep up to `nbytes` of freed scratch (default: all)."""
    _check(load_library().he_set_scratch_cache(nbytes))


def trim_scratch(keep_bytes=0):
    _check(load_library().he_device_trim_scratch(keep_bytes))


def scratch_cached_bytes():
    """Bytes of released scratch the library's cache holds on the current device (he_scratch_cached_bytes)."""
    out = c_u64(0)
    _check(load_library().he_scratch_cached_bytes(ctypes.byref(out)))
    return out.value


def shard_bounds(total, members, member):
    """he_shard_bounds: member `member` of `members` owns units [begin, end) of `total`."""
    begin, end = c_size(0), c_size(0)
    _check(load_library().he_shard_bounds(total, members, member, ctypes.byref(begin), ctypes.byref(end)))
    return begin.value, end.value


GROUP_STAGE_ALL = 1


class DeviceGroup:
    """he_device_group: one Context<Bfv<UInt64>> and one stream per member device of ONE process; the units of a call split
    over the members by shard_bounds, the finished shards gathered on member 0's device (include/he_amd.h "Device groups")."""

    def __init__(self, devices, degree, plaintext_modulus, coefficient_moduli, stage_all=False):
        ids = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        q = (c_u64 * len(coefficient_moduli))(*[int(m) for m in coefficient_moduli])
        handle = vp()
        _check(load_library().he_device_group_create(ids, len(devices), GROUP_STAGE_ALL if stage_all else 0, degree,
                                                     int(plaintext_modulus), q, len(coefficient_moduli), ctypes.byref(handle)))
        self.h = handle
        self.degree = degree
        self.devices = [int(d) for d in devices]
        self.L = len(coefficient_moduli) - 1 if len(coefficient_moduli) > 1 else 1

    def __del__(self):
        if getattr(self, "h", None):
            load_library().he_device_group_destroy(self.h)
            self.h = None

    def __len__(self):
        return int(load_library().he_device_group_size(self.h))

    def bounds(self, total, member):
        return shard_bounds(total, len(self), member)

    def stream(self, member):
        """The member's stream as a torch stream (owned by the group)."""
        import torch

        return torch.cuda.ExternalStream(int(load_library().he_device_group_stream(self.h, member)),
                                         device=self.devices[member])

    def synchronize(self):
        _check(load_library().he_device_group_synchronize(self.h))

    def _shards(self, tensors):
        return (vp * len(tensors))(*[vp(0) if t is None else vp(t.data_ptr()) for t in tensors])

    def forward_ntt_(self, slab_shards, batch, moduli_count=None):
        _check(load_library().he_ntt_forward_group(self.h, moduli_count or self.L, self._shards(slab_shards), batch))
        return slab_shards

    def inverse_ntt_(self, slab_shards, batch, moduli_count=None):
        _check(load_library().he_ntt_inverse_group(self.h, moduli_count or self.L, self._shards(slab_shards), batch))
        return slab_shards

    def pir_dim0_columns(self, dim0_query_eval, database_shards, columns, present_shards=None, stream=None):
        """he_pir_dim0_columns_group: database_shards[m] = member m's columns [share][d0][L][N] on its device; the result
        [columns][2][L][N] on member 0's device (where dim0_query_eval lives)."""
        import torch

        d0 = dim0_query_eval.numel() // (2 * self.L * self.degree)
        out = torch.empty((columns, 2, self.L, self.degree), dtype=dim0_query_eval.dtype, device=dim0_query_eval.device)
        masks = None if present_shards is None else self._shards(present_shards)
        _check(load_library().he_pir_dim0_columns_group(self.h, _ptr(dim0_query_eval), d0, self._shards(database_shards),
                                                        masks, columns, _ptr(out), _stream(stream)))
        return out

    def pir_compute_response(self, dimensions, dim0_query_eval, remaining_query, database_shards, chunk_count,
                             present_shards=None, relinearization_key=None, stream=None):
        """he_pir_compute_response_group: the chunk loop over the group; database_shards[m] = member m's share of the
        chunk_count x columns columns of all chunks -> [chunks][2][1][N] on member 0's device."""
        import torch

        dims = (c_u32 * len(dimensions))(*[int(d) for d in dimensions])
        out = torch.empty((chunk_count, 2, 1, self.degree), dtype=dim0_query_eval.dtype, device=dim0_query_eval.device)
        rest = vp() if remaining_query is None else _ptr(remaining_query)
        rest_count = 0 if remaining_query is None else remaining_query.numel() // (2 * self.L * self.degree)
        key = vp() if relinearization_key is None else _ptr(relinearization_key)
        masks = None if present_shards is None else self._shards(present_shards)
        _check(load_library().he_pir_compute_response_group(self.h, dims, len(dims), _ptr(dim0_query_eval), rest, rest_count,
                                                            self._shards(database_shards), masks, chunk_count, key,
                                                            _ptr(out), _stream(stream)))
        return out

    def pir_compute_response_chunk(self, dimensions, dim0_query_eval, remaining_query, database_shards,
                                   present_shards=None, relinearization_key=None, stream=None):
        """he_pir_compute_response_chunk_group -> [2][1][N] on member 0's device."""
        import torch

        dims = (c_u32 * len(dimensions))(*[int(d) for d in dimensions])
        out = torch.empty((2, 1, self.degree), dtype=dim0_query_eval.dtype, device=dim0_query_eval.device)
        rest = vp() if remaining_query is None else _ptr(remaining_query)
        rest_count = 0 if remaining_query is None else remaining_query.numel() // (2 * self.L * self.degree)
        key = vp() if relinearization_key is None else _ptr(relinearization_key)
        masks = None if present_shards is None else self._shards(present_shards)
        _check(load_library().he_pir_compute_response_chunk_group(self.h, dims, len(dims), _ptr(dim0_query_eval), rest,
                                                                  rest_count, self._shards(database_shards), masks, key,
                                                                  _ptr(out), _stream(stream)))
        return out


def stream_copy(src, dst, non_temporal=False, stream=None):
    """dst <- src with the library's streaming copy (8 bytes per lane): the roofline's reference rate."""
    _check(load_library().he_words_copy_device(vp(src.data_ptr()), vp(dst.data_ptr()), src.numel(),
                                               1 if non_temporal else 0, _stream(stream)))


def widen_u32(slab32, stream=None):
    """[UInt32] words (int32 tensor) -> zero-extended 8-byte words (int64 tensor of the same shape), on the device."""
    import torch

    out = torch.empty(slab32.shape, dtype=torch.int64, device=slab32.device)
    _check(load_library().he_words_widen_u32_device(vp(slab32.data_ptr()), vp(out.data_ptr()), slab32.numel(),
                                                    _stream(stream)))
    return out


def narrow_u64(slab64, stream=None):
    """8-byte words holding UInt32 values -> packed int32 tensor of the same shape."""
    import torch

    out = torch.empty(slab64.shape, dtype=torch.int32, device=slab64.device)
    _check(load_library().he_words_narrow_u64_device(vp(slab64.data_ptr()), vp(out.data_ptr()), slab64.numel(),
                                                     _stream(stream)))
    return out


def galois_element_swapping_rows(degree):
    out = ctypes.c_uint64(0)
    _check(load_library().he_galois_element_swapping_rows(degree, ctypes.byref(out)))
    return out.value


def galois_element_rotating_columns(step, degree):
    out = ctypes.c_uint64(0)
    _check(load_library().he_galois_element_rotating_columns(step, degree, ctypes.byref(out)))
    return out.value


def generate_primes(bit_counts, preferring_small, ntt_degree=1):
    bits = (ctypes.c_int32 * len(bit_counts))(*bit_counts)
    out = np.zeros(len(bit_counts), dtype=np.uint64)
    _check(load_library().he_generate_primes(bits, len(bit_counts), int(preferring_small), ntt_degree,
                                            out.ctypes.data_as(U64P)))
    return [int(v) for v in out]


def _u64(values):
    return np.ascontiguousarray(values, dtype=np.uint64)


def to_device(array, device="cuda"):
    """numpy uint64 array -> torch int64 CUDA tensor holding the same words."""
    import torch

    a = np.ascontiguousarray(array, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to(device)


def to_host(tensor):
    """torch int64 tensor -> numpy uint64 array (same words)."""
    return tensor.detach().cpu().contiguous().numpy().view(np.uint64)


def to_device32(array, device="cuda"):
    """numpy array of values < 2^32 -> torch int32 CUDA tensor holding them as packed UInt32 words."""
    import torch

    a = np.ascontiguousarray(array, dtype=np.uint64).astype(np.uint32)
    return torch.from_numpy(a.view(np.int32)).to(device)


def to_host32(tensor):
    """torch int32 tensor of packed UInt32 words -> numpy uint64 array of the values."""
    return tensor.detach().cpu().contiguous().numpy().view(np.uint32).astype(np.uint64)


def _entry(name, word=WORD64):
    """The C entry `name` for slabs of `word`."""
    return getattr(load_library(), name + word.suffix)


def _ptr(tensor, word=WORD64):
    if not tensor.is_cuda:
        raise ValueError("expected a CUDA (HIP) tensor")
    if not tensor.is_contiguous():
        raise ValueError("expected a contiguous tensor")
    if tensor.element_size() * 8 != word.bits:
        raise ValueError(f"expected {word.bits}-bit words ({word.dtype} storage)")
    return vp(tensor.data_ptr())


def _opt_ptr(tensor, word=WORD64):
    return vp() if tensor is None else _ptr(tensor, word)


def _empty(shape, word, device):
    import torch

    return torch.empty(shape, dtype=getattr(torch, word.dtype), device=device)


def _workspace(workspace):
    if workspace is None:
        return vp(), 0
    return vp(workspace.data_ptr()), workspace.numel() * workspace.element_size()


def _stream(stream):
    import torch

    if stream is None:
        stream = torch.cuda.current_stream()
    return vp(stream.cuda_stream)


class PolyContext:
    """PolyContext<UInt64> (reference PolyRq/PolyContext.swift:19-123) resident on the current GPU."""

    def __init__(self, degree, moduli, host_only=False, _borrowed=None, _keepalive=None):
        lib = load_library()
        self._owned = _borrowed is None
        self._keepalive = _keepalive
        if _borrowed is not None:
            self.h = vp(_borrowed)
        else:
            arr = _u64(list(moduli))
            h = vp()
            create = lib.he_poly_context_create_host_only if host_only else lib.he_poly_context_create
            _check(create(degree, arr.ctypes.data_as(U64P), len(arr), ctypes.byref(h)))
            self.h = h
        self.degree = int(lib.he_poly_context_degree(self.h))
        count = int(lib.he_poly_context_moduli_count(self.h))
        out = np.zeros(count, dtype=np.uint64)
        _check(lib.he_poly_context_moduli(self.h, out.ctypes.data_as(U64P)))
        self.moduli = [int(v) for v in out]

    def __del__(self):
        if getattr(self, "_owned", False) and getattr(self, "h", None) and _lib is not None:
            _lib.he_poly_context_destroy(self.h)
            self.h = None

    # ---- host-side queries
    def max_lazy_product_accumulation_count(self):
        return int(load_library().he_poly_context_max_lazy_product_accumulation_count(self.h))

    def q_remainder(self, modulus):
        out = c_u64(0)
        _check(load_library().he_poly_context_q_remainder(self.h, modulus, ctypes.byref(out)))
        return int(out.value)

    def ntt_tables(self, rns_index):
        n = self.degree
        arrs = [np.zeros(n, dtype=np.uint64) for _ in range(4)]
        inv_n, inv_n_root = c_u64(0), c_u64(0)
        _check(load_library().he_poly_context_copy_ntt_tables(
            self.h, rns_index, *[a.ctypes.data_as(U64P) for a in arrs], ctypes.byref(inv_n), ctypes.byref(inv_n_root)))
        return dict(root_powers=arrs[0], root_factors=arrs[1], inv_root_powers=arrs[2], inv_root_factors=arrs[3],
                    inverse_degree=int(inv_n.value), inverse_degree_root=int(inv_n_root.value))

    def _batch(self, tensor, rows=None):
        per = (len(self.moduli) if rows is None else rows) * self.degree
        if tensor.numel() % per:
            raise ValueError(f"slab of {tensor.numel()} words is not [batch][{per // self.degree}][{self.degree}]")
        return tensor.numel() // per

    # ---- PolyRq.forwardNtt / inverseNtt (in place, device tensors).  One body per operation takes the slab's word; the `_u32`
    # names are PolyRq<UInt32> on int32 tensors [batch][L][N] of packed UInt32 words.
    def _ntt(self, name, slab, word, stream):
        _check(_entry(name, word)(self.h, _ptr(slab, word), self._batch(slab), _stream(stream)))
        return slab

    def forward_ntt_(self, slab, stream=None):
        return self._ntt("he_ntt_forward_device", slab, WORD64, stream)

    def inverse_ntt_(self, slab, stream=None):
        return self._ntt("he_ntt_inverse_device", slab, WORD64, stream)

    def forward_ntt_u32_(self, slab, stream=None):
        return self._ntt("he_ntt_forward_device", slab, WORD32, stream)

    def inverse_ntt_u32_(self, slab, stream=None):
        return self._ntt("he_ntt_inverse_device", slab, WORD32, stream)

    def ntt_variant_(self, slab, inverse, variant, stream=None):
        _check(load_library().he_ntt_device_variant(self.h, _ptr(slab), self._batch(slab), int(inverse), variant,
                                                    _stream(stream)))
        return slab

    def forward_ntt_rows_(self, modulus, rows, stream=None):
        _check(load_library().he_ntt_forward_rows_device(self.h, modulus, _ptr(rows), rows.numel() // self.degree,
                                                         _stream(stream)))
        return rows

    def inverse_ntt_rows_(self, modulus, rows, stream=None):
        _check(load_library().he_ntt_inverse_rows_device(self.h, modulus, _ptr(rows), rows.numel() // self.degree,
                                                         _stream(stream)))
        return rows

    # host-pointer forms (numpy in, numpy out): the reference's borrowed-pointer seam
    def forward_ntt_host(self, array):
        out = _u64(array).copy()
        _check(load_library().he_ntt_forward(self.h, out.ctypes.data_as(U64P), self._batch_np(out)))
        return out

    def forward_ntt_host_(self, array):
        """In place on a host array (C-contiguous uint64): the call PolyRq.forwardNtt() on a host polynomial maps to."""
        assert array.dtype == np.uint64 and array.flags["C_CONTIGUOUS"] and array.flags["WRITEABLE"]
        _check(load_library().he_ntt_forward(self.h, array.ctypes.data_as(U64P), self._batch_np(array)))
        return array

    def inverse_ntt_host_(self, array):
        assert array.dtype == np.uint64 and array.flags["C_CONTIGUOUS"] and array.flags["WRITEABLE"]
        _check(load_library().he_ntt_inverse(self.h, array.ctypes.data_as(U64P), self._batch_np(array)))
        return array

    def inverse_ntt_host(self, array):
        out = _u64(array).copy()
        _check(load_library().he_ntt_inverse(self.h, out.ctypes.data_as(U64P), self._batch_np(out)))
        return out

    def _batch_np(self, array):
        per = len(self.moduli) * self.degree
        if array.size % per:
            raise ValueError("slab is not [batch][L][N]")
        return array.size // per

    # ---- element-wise (in place on lhs)
    def _binary(self, name, lhs, rhs, word, stream):
        _check(_entry(name, word)(self.h, _ptr(lhs, word), _ptr(rhs, word), self._batch(lhs), _stream(stream)))
        return lhs

    def _neg(self, data, word, stream):
        _check(_entry("he_poly_neg_device", word)(self.h, _ptr(data, word), self._batch(data), _stream(stream)))
        return data

    def _mul_scalar(self, data, scalar_residues, word, stream):
        if word is WORD32:  # the one entry whose twin differs: it takes uint32 residues
            residues = (c_u32 * len(self.moduli))(*[int(v) for v in scalar_residues])
        else:
            array = _u64(list(scalar_residues))
            residues = array.ctypes.data_as(U64P)
        _check(_entry("he_poly_mul_scalar_device", word)(self.h, _ptr(data, word), residues, self._batch(data),
                                                         _stream(stream)))
        return data

    def _divide_and_round_q_last(self, slab, word, stream):
        batch = self._batch(slab)
        out = _empty((batch, max(len(self.moduli) - 1, 0), self.degree), word, slab.device)
        _check(_entry("he_poly_divide_and_round_q_last_device", word)(self.h, _ptr(slab, word), vp(out.data_ptr()), batch,
                                                                      _stream(stream)))
        return out

    def add_(self, lhs, rhs, stream=None):
        return self._binary("he_poly_add_device", lhs, rhs, WORD64, stream)

    def sub_(self, lhs, rhs, stream=None):
        return self._binary("he_poly_sub_device", lhs, rhs, WORD64, stream)

    def neg_(self, data, stream=None):
        return self._neg(data, WORD64, stream)

    def mul_(self, lhs, rhs, stream=None):
        return self._binary("he_poly_mul_device", lhs, rhs, WORD64, stream)

    def elementwise_u32_(self, op, lhs, rhs=None, stream=None):
        if op == "neg":
            return self._neg(lhs, WORD32, stream)
        name = {"add": "he_poly_add_device", "sub": "he_poly_sub_device", "mul": "he_poly_mul_device"}[op]
        return self._binary(name, lhs, rhs, WORD32, stream)

    def mul_scalar_(self, data, scalar_residues, stream=None):
        return self._mul_scalar(data, scalar_residues, WORD64, stream)

    def mul_scalar_u32_(self, data, scalar_residues, stream=None):
        return self._mul_scalar(data, scalar_residues, WORD32, stream)

    def divide_and_round_q_last(self, slab, stream=None):
        return self._divide_and_round_q_last(slab, WORD64, stream)

    def divide_and_round_q_last_u32(self, slab, stream=None):
        return self._divide_and_round_q_last(slab, WORD32, stream)

    def divide_and_round_q_last_host(self, array):
        a = _u64(array)
        batch = self._batch_np(a)
        out = np.zeros((batch, len(self.moduli) - 1, self.degree), dtype=np.uint64)
        _check(load_library().he_poly_divide_and_round_q_last(self.h, a.ctypes.data_as(U64P),
                                                              out.ctypes.data_as(U64P), batch))
        return out

    # ---- the wire format of polynomials, on either word, and of whole ciphertexts ----
    def _random_from_seeds(self, seeds, word, stream):
        batch = seeds.numel() // 32
        out = _empty((batch, len(self.moduli), self.degree), word, seeds.device)
        _check(_entry("he_poly_random_from_seeds_device", word)(self.h, vp(seeds.data_ptr()), batch, vp(out.data_ptr()),
                                                                _stream(stream)))
        return out

    def _serialize(self, slab, skip_lsbs, word, stream):
        import torch

        batch = self._batch(slab)
        out = torch.empty((batch, self.serialization_byte_count(skip_lsbs)), dtype=torch.uint8, device=slab.device)
        _check(_entry("he_poly_serialize_device", word)(self.h, _ptr(slab, word), batch, skip_lsbs, vp(out.data_ptr()),
                                                        _stream(stream)))
        return out

    def _deserialize(self, data, skip_lsbs, word, stream):
        batch, per = data.shape[0], data.shape[1]
        out = _empty((batch, len(self.moduli), self.degree), word, data.device)
        _check(_entry("he_poly_deserialize_device", word)(self.h, vp(data.data_ptr()), per, batch, skip_lsbs,
                                                          vp(out.data_ptr()), _stream(stream)))
        return out

    def random_from_seeds(self, seeds, stream=None):
        """PolyRq.random(context:using: NistAes128Ctr(seed:)) per seed: uint8 tensor [batch][32] -> [batch][L][N]."""
        return self._random_from_seeds(seeds, WORD64, stream)

    def random_from_seeds_u32(self, seeds, stream=None):
        return self._random_from_seeds(seeds, WORD32, stream)

    def _sample_from_seeds(self, entry, seeds, word, stream):
        batch = seeds.numel() // 32
        out = _empty((batch, len(self.moduli), self.degree), word, seeds.device)
        _check(getattr(load_library(), entry)(self.h, word.bits, vp(seeds.data_ptr()), batch, vp(out.data_ptr()),
                                              _stream(stream)))
        return out

    def random_ternary_from_seeds(self, seeds, word=WORD64, stream=None):
        """randomizeTernary over NistAes128Ctr(seed:) per seed: uint8 tensor [batch][32] -> [batch][L][N] Coeff in `word`."""
        return self._sample_from_seeds("he_poly_random_ternary_from_seeds_device", seeds, word, stream)

    def random_centered_binomial_from_seeds(self, seeds, word=WORD64, stream=None):
        """randomizeCenteredBinomialDistribution (stdDev32) over NistAes128Ctr(seed:) per seed -> [batch][L][N] Coeff."""
        return self._sample_from_seeds("he_poly_random_centered_binomial_from_seeds_device", seeds, word, stream)

    def serialization_byte_count(self, skip_lsbs=0):
        return int(load_library().he_poly_serialization_byte_count(self.h, skip_lsbs))

    def serialize(self, slab, skip_lsbs=0, stream=None):
        """PolyRq.serialize per polynomial: [batch][L][N] -> uint8 tensor [batch][byte count]."""
        return self._serialize(slab, skip_lsbs, WORD64, stream)

    def serialize_u32(self, slab, skip_lsbs=0, stream=None):
        return self._serialize(slab, skip_lsbs, WORD32, stream)

    def deserialize(self, data, skip_lsbs=0, stream=None):
        """PolyRq(deserialize:context:skipLSBs:) per record: uint8 tensor [batch][bytes] -> [batch][L][N]."""
        return self._deserialize(data, skip_lsbs, WORD64, stream)

    def deserialize_u32(self, data, skip_lsbs=0, stream=None):
        return self._deserialize(data, skip_lsbs, WORD32, stream)

    @staticmethod
    def _skips(skip_lsbs, poly_count):
        if skip_lsbs is None:
            return None
        assert len(skip_lsbs) >= max(poly_count, 1)
        return (ctypes.c_int * len(skip_lsbs))(*[int(v) for v in skip_lsbs])

    def ciphertexts_serialization_byte_count(self, poly_count, skip_lsbs=None):
        return int(load_library().he_ciphertexts_serialization_byte_count(self.h, poly_count,
                                                                          self._skips(skip_lsbs, poly_count)))

    def ciphertexts_wire_plan(self, direction, poly_count, skip_lsbs=None, record_stride=0, records_address=0,
                              slab_address=0, word_bits=64):
        """he_ciphertexts_wire_plan -> dict(form, record_bytes, items_per_record, edge_free).  Host only."""
        form, edge = c_u32(0), c_u32(0)
        record_bytes, items = c_size(0), c_size(0)
        _check(load_library().he_ciphertexts_wire_plan(
            {"serialize": 0, "deserialize": 1}[direction], word_bits, self.h, poly_count, self._skips(skip_lsbs, poly_count),
            record_stride, records_address, slab_address, ctypes.byref(form), ctypes.byref(record_bytes), ctypes.byref(items),
            ctypes.byref(edge)))
        names = {0: "byte", 1: "word", 2: "tile", 3: "chunk", 4: "field"}
        return {"form": names[form.value], "record_bytes": record_bytes.value, "items_per_record": items.value,
                "edge_free": bool(edge.value)}

    def ciphertexts_serialize(self, cts, skip_lsbs=None, record_stride=None, out=None, stream=None):
        """Ciphertext.serialize(forDecryption:) per ciphertext: [count][polys][L][N] (int64, or int32 for the _u32 entry) ->
        uint8 records `record_stride` bytes apart, written into `out` from its first byte when given."""
        import torch

        count, polys = cts.shape[0], cts.shape[1]
        need = self.ciphertexts_serialization_byte_count(polys, skip_lsbs)
        stride = need if record_stride is None else record_stride
        if out is None:
            out = torch.empty((count, stride), dtype=torch.uint8, device=cts.device)
        fn = _entry("he_ciphertexts_serialize_device", WORD32 if cts.dtype == torch.int32 else WORD64)
        _check(fn(self.h, vp(cts.data_ptr()), count, polys, self._skips(skip_lsbs, polys), vp(out.data_ptr()), stride,
                  _stream(stream)))
        return out

    def ciphertexts_deserialize(self, records, count, poly_count, skip_lsbs=None, record_stride=None, word_bits=64, out=None,
                                mismatch=None, stream=None):
        """Ciphertext(deserialize: .full) per record -> [count][polys][L][N]; mismatch: a zeroed int32 device tensor."""
        word = _word_of(word_bits)
        stride = self.ciphertexts_serialization_byte_count(poly_count, skip_lsbs) if record_stride is None else record_stride
        if out is None:
            out = _empty((count, poly_count, len(self.moduli), self.degree), word, records.device)
        _check(_entry("he_ciphertexts_deserialize_device", word)(
            self.h, vp(records.data_ptr()), stride, count, poly_count, self._skips(skip_lsbs, poly_count),
            vp(out.data_ptr()), None if mismatch is None else vp(mismatch.data_ptr()), _stream(stream)))
        return out

    def ciphertexts_deserialize_seeded(self, poly0_bytes, seeds, count, coeff_format, record_stride=None, word_bits=64,
                                       out=None, stream=None):
        """Ciphertext(deserialize: .seeded(poly0:seed:)) per ciphertext -> [count][2][L][N]; either input may be None."""
        word = _word_of(word_bits)
        stride = self.serialization_byte_count(0) if record_stride is None else record_stride
        if out is None:
            device = (poly0_bytes if poly0_bytes is not None else seeds).device
            out = _empty((count, 2, len(self.moduli), self.degree), word, device)
        _check(_entry("he_ciphertexts_deserialize_seeded_device", word)(
            self.h, None if poly0_bytes is None else vp(poly0_bytes.data_ptr()), stride,
            None if seeds is None else vp(seeds.data_ptr()), count, int(bool(coeff_format)), vp(out.data_ptr()),
            _stream(stream)))
        return out

    def apply_galois(self, slab, element, eval_format=False, stream=None):
        """PolyRq.applyGalois(element:) on [batch][L][N]; returns a new slab (the permutation is out of place)."""
        import torch

        out = torch.empty_like(slab)
        _check(load_library().he_poly_apply_galois_device(self.h, _ptr(slab), vp(out.data_ptr()), self._batch(slab),
                                                          int(element), int(bool(eval_format)), _stream(stream)))
        return out

    def multiply_power_of_x(self, slab, power, stream=None):
        """PolyRq<Coeff>.multiplyPowerOfX(power); returns a new slab."""
        import torch

        out = torch.empty_like(slab)
        _check(load_library().he_poly_multiply_power_of_x_device(self.h, _ptr(slab), vp(out.data_ptr()),
                                                                 self._batch(slab), int(power), _stream(stream)))
        return out

    def adding_lazy_product_(self, lhs, rhs, acc, stream=None):
        _check(load_library().he_poly_adding_lazy_product_device(self.h, _ptr(lhs), _ptr(rhs), _ptr(acc),
                                                                 _stream(stream)))
        return acc

    def reduce_accumulator(self, acc, stream=None):
        import torch

        out = torch.empty((len(self.moduli), self.degree), dtype=torch.int64, device=acc.device)
        _check(load_library().he_poly_reduce_accumulator_device(self.h, _ptr(acc), vp(out.data_ptr()), _stream(stream)))
        return out


class BfvContext:
    """Context<Bfv<UInt64>> (reference Context.swift:94-159) plus the Bfv operations on the hot path.  Each method resolves
    its entry, checks its slabs and allocates its result through the class's slab word; a method whose entry has no 4-byte
    twin names WORD64 and works on 8-byte slabs in BfvContext32 too."""

    _word = WORD64  # of the class, not of word_bits: BfvContext(word_bits=32) holds Bfv<UInt32> constants on 8-byte slabs

    def __init__(self, degree, plaintext_modulus, coefficient_moduli, host_only=False, word_bits=64):
        """word_bits=32: Context<Bfv<UInt32>> constants on 8-byte words (he_bfv_context_create_u32)."""
        lib = load_library()
        arr = _u64(list(coefficient_moduli))
        h = vp()
        word = _word_of(word_bits)  # of the constants; the slabs' word is the class's
        host = host_only and word is WORD64
        create = lib.he_bfv_context_create_host_only if host else _entry("he_bfv_context_create", word)
        _check(create(degree, plaintext_modulus, arr.ctypes.data_as(U64P), len(arr), ctypes.byref(h)))
        self.h = h
        self.degree = degree
        self.word_bits = word_bits
        self.t = plaintext_modulus
        self.coefficient_moduli = [int(v) for v in arr]
        self.L = int(lib.he_bfv_ciphertext_moduli_count(self.h))

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.he_bfv_context_destroy(self.h)
            self.h = None

    def _L(self, moduli_count):
        return self.L if moduli_count is None else moduli_count

    def _sub(self, getter, moduli_count):
        handle = getter(self.h, self._L(moduli_count))
        if not handle:
            raise HeError(16, "moduli_count out of range")
        return PolyContext(None, None, _borrowed=handle, _keepalive=self)

    def ciphertext_context(self, moduli_count=None):
        return self._sub(load_library().he_bfv_ciphertext_context, moduli_count)

    def key_switching_context(self, moduli_count=None):
        return self._sub(load_library().he_bfv_key_switching_context, moduli_count)

    def qbsk_context(self, moduli_count=None):
        return self._sub(load_library().he_bfv_qbsk_context, moduli_count)

    def bsk_moduli(self):
        out = np.zeros(self.L + 1, dtype=np.uint64)
        _check(load_library().he_bfv_copy_bsk_moduli(self.h, out.ctypes.data_as(U64P)))
        return [int(v) for v in out]

    def lift_q_to_qbsk(self, polys, moduli_count=None, stream=None):
        L, w = self._L(moduli_count), self._word
        batch = polys.numel() // (L * self.degree)
        out = _empty((batch, 2 * L + 1, self.degree), w, polys.device)
        _check(_entry("he_rns_lift_q_to_qbsk_device", w)(
            self.h, L, _ptr(polys, w), _ptr(out, w), batch, _stream(stream)))
        return out

    def floor_qbsk_to_q(self, polys, moduli_count=None, stream=None):
        L, w = self._L(moduli_count), self._word
        batch = polys.numel() // ((2 * L + 1) * self.degree)
        out = _empty((batch, L, self.degree), w, polys.device)
        _check(_entry("he_rns_floor_qbsk_to_q_device", w)(
            self.h, L, _ptr(polys, w), _ptr(out, w), batch, _stream(stream)))
        return out

    def mul(self, lhs, rhs, moduli_count=None, stream=None, workspace=None):
        """Bfv.mulAssign(ct, ct): [batch][2][L][N] x [batch][2][L][N] -> [batch][3][L][N] (Coeff)."""
        L, w = self._L(moduli_count), self._word
        batch = lhs.numel() // (2 * L * self.degree)
        out = _empty((batch, 3, L, self.degree), w, lhs.device)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(_entry("he_bfv_mul_device", w)(
            self.h, L, _ptr(lhs, w), _ptr(rhs, w), _ptr(out, w), batch, ws_ptr, ws_bytes, _stream(stream)))
        return out

    def mul_workspace_bytes(self, batch, moduli_count=None):
        return int(load_library().he_bfv_mul_workspace_bytes(self.h, self._L(moduli_count), batch))

    def relinearize_workspace_bytes(self, batch, moduli_count=None):
        return int(load_library().he_bfv_relinearize_workspace_bytes(self.h, self._L(moduli_count), batch))

    def relinearize(self, ct3, key, moduli_count=None, stream=None, workspace=None):
        """Bfv.relinearize: [batch][3][L][N] + key [L_top][2][L_top+1][N] -> [batch][2][L][N]."""
        L, w = self._L(moduli_count), self._word
        batch = ct3.numel() // (3 * L * self.degree)
        out = _empty((batch, 2, L, self.degree), w, ct3.device)
        key_ptr = _opt_ptr(key, w)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(_entry("he_bfv_relinearize_device", w)(
            self.h, L, _ptr(ct3, w), key_ptr, _ptr(out, w), batch, ws_ptr, ws_bytes, _stream(stream)))
        return out

    def apply_galois_workspace_bytes(self, batch, moduli_count=None):
        return int(load_library().he_bfv_apply_galois_workspace_bytes(self.h, self._L(moduli_count), batch))

    def apply_galois(self, ct, element, key, moduli_count=None, stream=None, workspace=None):
        """Bfv.applyGalois: [batch][2][L][N] Coeff + the element's Galois key -> [batch][2][L][N]."""
        L, w = self._L(moduli_count), self._word
        batch = ct.numel() // (2 * L * self.degree)
        out = _empty((batch, 2, L, self.degree), w, ct.device)
        key_ptr = _opt_ptr(key, w)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(_entry("he_bfv_apply_galois_device", w)(
            self.h, L, _ptr(ct, w), int(element), key_ptr, _ptr(out, w), batch, ws_ptr, ws_bytes, _stream(stream)))
        return out

    def scale_and_round(self, poly, scaling_factor=1, moduli_count=None, stream=None):
        """_RnsTool.scaleAndRound: [batch][L][N] Coeff -> [batch][N] mod t."""
        L, w = self._L(moduli_count), self._word
        batch = poly.numel() // (L * self.degree)
        out = _empty((batch, self.degree), w, poly.device)
        _check(_entry("he_rns_scale_and_round_device", w)(
            self.h, L, _ptr(poly, w), int(scaling_factor), _ptr(out, w), batch, _stream(stream)))
        return out

    def plaintext_to_eval(self, plaintext, moduli_count=None, stream=None):
        """Plaintext.convertToEvalFormat: [batch][N] (values < t) -> [batch][L][N] Eval."""
        L, w = self._L(moduli_count), self._word
        batch = plaintext.numel() // self.degree
        out = _empty((batch, L, self.degree), w, plaintext.device)
        _check(_entry("he_bfv_plaintext_to_eval_device", w)(
            self.h, L, _ptr(plaintext, w), _ptr(out, w), batch, _stream(stream)))
        return out

    def plaintext_to_coeff(self, plaintext_eval, moduli_count=None, stream=None):
        """Plaintext.convertToCoeffFormat: [batch][L][N] Eval -> [batch][N] (values < t)."""
        L, w = self._L(moduli_count), self._word
        batch = plaintext_eval.numel() // (L * self.degree)
        out = _empty((batch, self.degree), w, plaintext_eval.device)
        _check(_entry("he_bfv_plaintext_to_coeff_device", w)(
            self.h, L, _ptr(plaintext_eval, w), _ptr(out, w), batch, _stream(stream)))
        return out

    # ---- decryption of resident ciphertexts.  cts: [batch][polys][L][N] in the class's slab word, Coeff form unless
    # eval_format; secret_key: [L_all][N] Eval over every coefficient modulus (its first L rows are read).
    @staticmethod
    def _ciphertext_shape(cts):
        if cts.dim() != 4:
            raise ValueError("expected ciphertexts as [batch][polys][L][N]")
        return cts.shape[0], cts.shape[1], cts.shape[2]

    def decrypt_workspace_bytes(self, batch, poly_count=2, eval_format=False, moduli_count=None):
        return int(load_library().he_bfv_decrypt_workspace_bytes(
            self.h, self._word.bits, self._L(moduli_count), poly_count, int(eval_format), batch))

    def secret_dot_product(self, cts, secret_key, eval_format=False, stream=None, workspace=None):
        """Bfv.dotProduct: c0 + c1 s [+ c2 s^2] -> [batch][L][N] Coeff."""
        (batch, polys, L), w = self._ciphertext_shape(cts), self._word
        out = _empty((batch, L, self.degree), w, cts.device)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(load_library().he_bfv_secret_dot_product_device(
            self.h, w.bits, L, polys, int(eval_format), _ptr(cts, w), _ptr(secret_key, w), _ptr(out, w), batch, ws_ptr,
            ws_bytes, _stream(stream)))
        return out

    def decrypt(self, cts, secret_key, correction_factor=1, eval_format=False, stream=None, workspace=None):
        """Bfv.decryptCoeff / decryptEval -> [batch][N], values < t."""
        (batch, polys, L), w = self._ciphertext_shape(cts), self._word
        out = _empty((batch, self.degree), w, cts.device)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(load_library().he_bfv_decrypt_device(
            self.h, w.bits, L, polys, int(eval_format), _ptr(cts, w), _ptr(secret_key, w), int(correction_factor),
            _ptr(out, w), batch, ws_ptr, ws_bytes, _stream(stream)))
        return out

    def noise_norm_limbs(self, moduli_count=None):
        return int(load_library().he_bfv_noise_norm_limbs(self.h, self._L(moduli_count)))

    def noise_norm_device(self, cts, secret_key, eval_format=False, stream=None, workspace=None):
        """max_k |[t (c0 + c1 s + ..)_k]_Q| per ciphertext -> [batch][limbs] little-endian 64-bit limbs (int64), enqueue-only."""
        (batch, polys, L), w = self._ciphertext_shape(cts), self._word
        out = _empty((batch, self.noise_norm_limbs(L)), WORD64, cts.device)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(load_library().he_bfv_noise_norm_device(
            self.h, w.bits, L, polys, int(eval_format), _ptr(cts, w), _ptr(secret_key, w), _ptr(out), batch, ws_ptr, ws_bytes,
            _stream(stream)))
        return out

    def noise_norm(self, cts, secret_key, eval_format=False, stream=None, workspace=None):
        """The same as Python integers (synchronises)."""
        limbs = self.noise_norm_device(cts, secret_key, eval_format, stream, workspace)
        if stream is not None:
            stream.synchronize()
        return [sum(int(limb) << (64 * i) for i, limb in enumerate(row)) for row in to_host(limbs).reshape(limbs.shape)]

    def noise_budget_from_norm(self, norm, moduli_count=None, variable_time=True):
        """Bfv.noiseBudget's last step for one norm (host only).  Never forward a noise budget to another party."""
        L = self._L(moduli_count)
        limbs = _u64([(int(norm) >> (64 * i)) & (2**64 - 1) for i in range(self.noise_norm_limbs(L))])
        out = ctypes.c_double(0.0)
        _check(load_library().he_bfv_noise_budget_from_norm(
            self.h, self.word_bits, L, limbs.ctypes.data_as(U64P), int(variable_time), ctypes.byref(out)))
        return out.value

    def noise_budget(self, cts, secret_key, eval_format=False, variable_time=True, stream=None, workspace=None):
        """Bfv.noiseBudgetCoeff / noiseBudgetEval per ciphertext -> floats (synchronises).  Never forward a noise budget to
        another party: sharing it acts as an oracle that can be used to recover the secret key."""
        L = self._ciphertext_shape(cts)[2]
        return [self.noise_budget_from_norm(norm, L, variable_time)
                for norm in self.noise_norm(cts, secret_key, eval_format, stream, workspace)]

    def is_transparent(self, cts, stream=None):
        """Bfv.isTransparent per ciphertext -> [batch] uint8 (1: every polynomial but the first is zero)."""
        import torch

        (batch, polys, L), w = self._ciphertext_shape(cts), self._word
        out = torch.empty((batch,), dtype=torch.uint8, device=cts.device)
        _check(load_library().he_bfv_is_transparent_device(
            self.h, w.bits, L, polys, _ptr(cts, w), vp(out.data_ptr()), batch, _stream(stream)))
        return out

    # ---- secret keys, encryption and evaluation keys from caller-supplied seeds (uint8 tensors [..][32] on the device; the
    # library generates none: draw them from os.urandom).  Error and key seeds are as secret as the key.
    ENCRYPT_OPERATIONS = {"secret_key": 0, "encrypt_zero": 1, "encrypt": 2, "key_switch_keys": 3, "relinearization_key": 4,
                          "galois_keys": 5}

    @property
    def coefficient_moduli_count(self):
        return len(self.coefficient_moduli)

    def encrypt_workspace_bytes(self, operation, count=1, moduli_count=None, eval_out=False):
        return int(load_library().he_bfv_encrypt_workspace_bytes(
            self.h, self._word.bits, self.ENCRYPT_OPERATIONS[operation], self._L(moduli_count), int(eval_out), count))

    def generate_secret_key(self, seeds, stream=None, workspace=None):
        """Bfv.generateSecretKey per seed -> [batch][L_all][N] Eval; one key is what decrypt and encrypt take."""
        batch, w = seeds.numel() // 32, self._word
        out = _empty((batch, self.coefficient_moduli_count, self.degree), w, seeds.device)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(load_library().he_bfv_generate_secret_key_device(
            self.h, w.bits, vp(seeds.data_ptr()), _ptr(out, w), batch, ws_ptr, ws_bytes, _stream(stream)))
        return out

    def encrypt_zero(self, secret_key, a_seeds, error_seeds, moduli_count=None, eval_out=False, stream=None, workspace=None):
        """Bfv.encryptZero over the first moduli_count coefficient moduli (up to L_all) -> [batch][2][m][N]."""
        batch, m, w = a_seeds.numel() // 32, self._L(moduli_count), self._word
        out = _empty((batch, 2, m, self.degree), w, a_seeds.device)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(load_library().he_bfv_encrypt_zero_device(
            self.h, w.bits, m, int(eval_out), _ptr(secret_key, w), vp(a_seeds.data_ptr()), vp(error_seeds.data_ptr()),
            _ptr(out, w), batch, ws_ptr, ws_bytes, _stream(stream)))
        return out

    def encrypt(self, plaintexts, secret_key, a_seeds, error_seeds, moduli_count=None, stream=None, workspace=None):
        """Bfv.encrypt: plaintexts [batch][N] (values < t) -> [batch][2][L][N] Coeff; a_seeds[b] is ciphertext b's seed."""
        batch, m, w = a_seeds.numel() // 32, self._L(moduli_count), self._word
        out = _empty((batch, 2, m, self.degree), w, a_seeds.device)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(load_library().he_bfv_encrypt_device(
            self.h, w.bits, m, _ptr(secret_key, w), vp(a_seeds.data_ptr()), vp(error_seeds.data_ptr()), _ptr(plaintexts, w),
            _ptr(out, w), batch, ws_ptr, ws_bytes, _stream(stream)))
        return out

    def generate_key_switch_keys(self, secret_key, current_keys, a_seeds, error_seeds, stream=None, workspace=None):
        """Bfv._generateKeySwitchKey: current_keys [keys][L+1][N] Eval, seeds [keys][L][32] -> [keys][L][2][L+1][N] Eval."""
        keys, w = current_keys.numel() // ((self.L + 1) * self.degree), self._word
        out = _empty((keys, self.L, 2, self.L + 1, self.degree), w, current_keys.device)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(load_library().he_bfv_generate_key_switch_keys_device(
            self.h, w.bits, _ptr(secret_key, w), _ptr(current_keys, w), vp(a_seeds.data_ptr()), vp(error_seeds.data_ptr()),
            _ptr(out, w), keys, ws_ptr, ws_bytes, _stream(stream)))
        return out

    def generate_relinearization_key(self, secret_key, a_seeds, error_seeds, stream=None, workspace=None):
        """Bfv.generateRelinearizationKey: seeds [L][32] -> [L][2][L+1][N] Eval, what relinearize takes."""
        w = self._word
        out = _empty((self.L, 2, self.L + 1, self.degree), w, secret_key.device)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(load_library().he_bfv_generate_relinearization_key_device(
            self.h, w.bits, _ptr(secret_key, w), vp(a_seeds.data_ptr()), vp(error_seeds.data_ptr()), _ptr(out, w), ws_ptr,
            ws_bytes, _stream(stream)))
        return out

    def generate_galois_keys(self, secret_key, elements, a_seeds, error_seeds, stream=None, workspace=None):
        """The Galois keys of Bfv.generateEvaluationKey: seeds [elements][L][32] -> [elements][L][2][L+1][N] Eval, slice e the
        key apply_galois takes for elements[e]."""
        w, element_array = self._word, _u64(list(elements))
        out = _empty((len(element_array), self.L, 2, self.L + 1, self.degree), w, secret_key.device)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(load_library().he_bfv_generate_galois_keys_device(
            self.h, w.bits, _ptr(secret_key, w), element_array.ctypes.data_as(U64P), len(element_array),
            vp(a_seeds.data_ptr()), vp(error_seeds.data_ptr()), _ptr(out, w), ws_ptr, ws_bytes, _stream(stream)))
        return out

    def pir_expand(self, ciphertexts, output_count, galois_keys, stream=None):
        """PirUtil.expand: [count][2][L][N] Coeff + {element: key tensor} -> [output_count][2][L][N]."""
        count = ciphertexts.numel() // (2 * self.L * self.degree)
        out = _empty((output_count, 2, self.L, self.degree), WORD64, ciphertexts.device)
        elements = sorted(galois_keys)
        element_array = _u64(elements)
        key_array = (vp * max(len(elements), 1))(*[vp(galois_keys[e].data_ptr()) for e in elements])
        _check(load_library().he_pir_expand_device(self.h, _ptr(ciphertexts), count, output_count,
                                                   element_array.ctypes.data_as(U64P), key_array, len(elements),
                                                   _ptr(out), _stream(stream)))
        return out

    def pir_expand_batch(self, ciphertexts, output_count, galois_keys_per_query, stream=None):
        """`queries` expansions of one shape: ciphertexts [queries][count][2][L][N]; galois_keys_per_query: one
        {element: key tensor} dict per query (the same elements in each) -> [queries][output_count][2][L][N]."""
        queries = len(galois_keys_per_query)
        count = ciphertexts.numel() // (queries * 2 * self.L * self.degree)
        out = _empty((queries, output_count, 2, self.L, self.degree), WORD64, ciphertexts.device)
        elements = sorted(galois_keys_per_query[0])
        element_array = _u64(elements)
        pointers = [vp(keys[e].data_ptr()) for keys in galois_keys_per_query for e in elements]
        key_array = (vp * max(len(pointers), 1))(*pointers)
        _check(load_library().he_pir_expand_batch_device(self.h, _ptr(ciphertexts), queries, count, output_count,
                                                         element_array.ctypes.data_as(U64P), key_array, len(elements),
                                                         _ptr(out), _stream(stream)))
        return out

    def pir_compute_response_chunk(self, dimensions, dim0_query_eval, remaining_query, database, present=None,
                                   relinearization_key=None, stream=None):
        """PirUtilProtocol.computeResponseForOneChunk -> response ciphertext [2][1][N] (Coeff, one modulus)."""
        dims = (c_u32 * len(dimensions))(*[int(d) for d in dimensions])
        out = _empty((2, 1, self.degree), WORD64, dim0_query_eval.device)
        pres = None
        if present is not None:
            pres_arr = np.ascontiguousarray(present, dtype=np.uint8)
            pres = pres_arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        rest = _opt_ptr(remaining_query)
        rest_count = 0 if remaining_query is None else remaining_query.numel() // (2 * self.L * self.degree)
        key = _opt_ptr(relinearization_key)
        _check(load_library().he_pir_compute_response_chunk_device(self.h, dims, len(dimensions),
                                                                   _ptr(dim0_query_eval), rest, rest_count,
                                                                   _ptr(database), pres, key, _ptr(out),
                                                                   _stream(stream)))
        return out

    def pir_dim0_columns(self, dim0_query_eval, database, present_device=None, stream=None):
        """PirUtil.swift:428-446 for a column shard: database [columns][d0][L][N] Eval -> [columns][2][L][N] Coeff.
        present_device: uint8 device tensor [columns][d0] or None.  Enqueue-only."""
        d0 = dim0_query_eval.numel() // (2 * self.L * self.degree)
        columns = database.numel() // (d0 * self.L * self.degree)
        out = _empty((columns, 2, self.L, self.degree), WORD64, dim0_query_eval.device)
        mask = vp() if present_device is None else vp(present_device.data_ptr())
        _check(load_library().he_pir_dim0_columns_device(self.h, _ptr(dim0_query_eval), d0, _ptr(database), mask,
                                                         columns, _ptr(out), _stream(stream)))
        return out

    def pir_remaining_dimensions(self, dimensions, intermediate, remaining_query, relinearization_key=None, stream=None):
        """PirUtil.swift:448-485 on all columns' dim-0 results ([columns][2][L][N] Coeff, consumed) -> [2][1][N]."""
        dims = (c_u32 * len(dimensions))(*[int(d) for d in dimensions])
        out = _empty((2, 1, self.degree), WORD64, intermediate.device)
        rest = _opt_ptr(remaining_query)
        rest_count = 0 if remaining_query is None else remaining_query.numel() // (2 * self.L * self.degree)
        key = _opt_ptr(relinearization_key)
        _check(load_library().he_pir_remaining_dimensions_device(self.h, dims, len(dimensions), _ptr(intermediate), rest,
                                                                 rest_count, key, _ptr(out), _stream(stream)))
        return out

    def pir_compute_response(self, dimensions, dim0_query_eval, remaining_query, database, chunk_count,
                             present_device=None, relinearization_key=None, stream=None):
        """PirUtil.computeResponse's chunk loop for one query: database [chunks][prod(dims)][L][N] -> [chunks][2][1][N]."""
        w = self._word
        dims = (c_u32 * len(dimensions))(*[int(d) for d in dimensions])
        out = _empty((chunk_count, 2, 1, self.degree), w, dim0_query_eval.device)
        rest = _opt_ptr(remaining_query, w)
        rest_count = 0 if remaining_query is None else remaining_query.numel() // (2 * self.L * self.degree)
        key = _opt_ptr(relinearization_key, w)
        mask = vp() if present_device is None else vp(present_device.data_ptr())
        _check(_entry("he_pir_compute_response_device", w)(
            self.h, dims, len(dimensions), _ptr(dim0_query_eval, w), rest, rest_count, _ptr(database, w), mask,
            chunk_count, key, _ptr(out, w), _stream(stream)))
        return out

    def pir_compute_response_to_query(self, dimensions, query_ciphertexts, indices_count, galois_keys, relinearization_key,
                                      databases, chunk_count, present_devices=None, stream=None):
        """PirUtil.computeResponse: Query.ciphertexts [count][2][L][N] Coeff + the evaluation key ({element: Galois key
        tensor}, relinearization key tensor or None) + one database tensor (shared by all indices) or a list of one per
        index (present_devices likewise: None, one mask or a list) -> [indices][chunks][2][1][N].  The Galois keys are 8-byte
        (widened) tensors on either slab word."""
        w = self._word
        dims = (c_u32 * len(dimensions))(*[int(d) for d in dimensions])
        count = query_ciphertexts.numel() // (2 * self.L * self.degree)
        out = _empty((indices_count, chunk_count, 2, 1, self.degree), w, query_ciphertexts.device)
        elements = sorted(galois_keys)
        element_array = _u64(elements)
        key_array = (vp * max(len(elements), 1))(*[vp(galois_keys[e].data_ptr()) for e in elements])
        relin = _opt_ptr(relinearization_key, w)
        database_list = list(databases) if isinstance(databases, (list, tuple)) else [databases]
        database_array = (vp * len(database_list))(*[vp(d.data_ptr()) for d in database_list])
        mask_array = None
        if present_devices is not None:
            mask_list = list(present_devices) if isinstance(present_devices, (list, tuple)) else [present_devices]
            mask_array = (vp * len(mask_list))(*[vp() if m is None else vp(m.data_ptr()) for m in mask_list])
        _check(_entry("he_pir_compute_response_to_query_device", w)(
            self.h, dims, len(dimensions), _ptr(query_ciphertexts, w), count, indices_count,
            element_array.ctypes.data_as(U64P), key_array, len(elements), relin, database_array, mask_array,
            len(database_list), chunk_count, _ptr(out, w), _stream(stream)))
        return out

    def pir_compute_response_queries(self, dimensions, dim0_queries_eval, remaining_queries, database, chunk_count,
                                     relinearization_keys, present_device=None, stream=None):
        """`queries` queries over one database in one call: dim0_queries_eval [d0][queries][2][L][N] Eval,
        remaining_queries [queries][rest][2][L][N] (or None), relinearization_keys: one tensor per query (or None)
        -> [queries][chunks][2][1][N]."""
        w = self._word
        dims = (c_u32 * len(dimensions))(*[int(d) for d in dimensions])
        queries = dim0_queries_eval.numel() // (int(dimensions[0]) * 2 * self.L * self.degree)
        out = _empty((queries, chunk_count, 2, 1, self.degree), w, dim0_queries_eval.device)
        rest = _opt_ptr(remaining_queries, w)
        rest_count = 0 if remaining_queries is None else remaining_queries.numel() // (queries * 2 * self.L * self.degree)
        keys = None
        if relinearization_keys is not None:
            keys = (vp * queries)(*[vp(k.data_ptr()) for k in relinearization_keys])
        mask = vp() if present_device is None else vp(present_device.data_ptr())
        _check(_entry("he_pir_compute_response_queries_device", w)(
            self.h, dims, len(dimensions), queries, _ptr(dim0_queries_eval, w), rest, rest_count, _ptr(database, w),
            mask, chunk_count, keys, _ptr(out, w), _stream(stream)))
        return out

    def mod_switch_down(self, ct, poly_count, moduli_count=None, stream=None):
        L, w = self._L(moduli_count), self._word
        batch = ct.numel() // (poly_count * L * self.degree)
        out = _empty((batch, poly_count, L - 1, self.degree), w, ct.device)
        _check(_entry("he_bfv_mod_switch_down_device", w)(
            self.h, L, poly_count, _ptr(ct, w), _ptr(out, w), batch, _stream(stream)))
        return out

    def mod_switch_down_to_single(self, ct, poly_count, moduli_count=None, stream=None):
        """Ciphertext.modSwitchDownToSingle: [batch][polys][L][N] -> [batch][polys][1][N]."""
        L = self._L(moduli_count)
        batch = ct.numel() // (poly_count * L * self.degree)
        out = _empty((batch, poly_count, 1, self.degree), WORD64, ct.device)
        _check(load_library().he_bfv_mod_switch_down_to_single_device(self.h, L, poly_count, _ptr(ct), _ptr(out), batch,
                                                                      _stream(stream)))
        return out

    def mul_plain_(self, ct, pt, poly_count, moduli_count=None, stream=None):
        L, w = self._L(moduli_count), self._word
        batch = pt.numel() // (L * self.degree)
        _check(_entry("he_bfv_mul_plain_device", w)(
            self.h, L, poly_count, _ptr(ct, w), _ptr(pt, w), batch, _stream(stream)))
        return ct

    def add_plain_(self, ct, plaintexts, poly_count=2, subtract=False, moduli_count=None, stream=None):
        """Bfv.addAssignCoeff / subAssignCoeff(ciphertext, plaintext): ct [batch][polys][L][N] Coeff in place,
        plaintexts [batch][N] mod t."""
        L, w = self._L(moduli_count), self._word
        batch = plaintexts.numel() // self.degree
        fn = _entry("he_bfv_sub_plain_device", w) if subtract else _entry("he_bfv_add_plain_device", w)
        _check(fn(self.h, L, poly_count, _ptr(ct, w), _ptr(plaintexts, w), batch, _stream(stream)))
        return ct

    def inner_product_plain(self, cts, pts, present=None, poly_count=2, columns=1, moduli_count=None, stream=None):
        """cts [count][polys][L][N]; pts [columns][count][L][N]; present: host bytes [columns][count] or None."""
        L = self._L(moduli_count)
        count = cts.numel() // (poly_count * L * self.degree)
        out = _empty((columns, poly_count, L, self.degree), WORD64, cts.device)
        pres = None
        if present is not None:
            pres_arr = np.ascontiguousarray(present, dtype=np.uint8)
            pres = pres_arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        _check(load_library().he_bfv_inner_product_plain_device(self.h, L, poly_count, _ptr(cts), _ptr(pts), pres,
                                                                count, columns, _ptr(out), _stream(stream)))
        return out

    def inner_product_plain_resident(self, cts, pts, present_device=None, poly_count=2, columns=1, moduli_count=None,
                                     stream=None):
        """inner_product_plain with the nil-plaintext mask as a uint8 DEVICE tensor [columns][count]: enqueue-only."""
        L, w = self._L(moduli_count), self._word
        count = cts.numel() // (poly_count * L * self.degree)
        out = _empty((columns, poly_count, L, self.degree), w, cts.device)
        mask = vp() if present_device is None else vp(present_device.data_ptr())
        _check(_entry("he_bfv_inner_product_plain_resident_device", w)(
            self.h, L, poly_count, _ptr(cts, w), _ptr(pts, w), mask, count, columns, _ptr(out, w), _stream(stream)))
        return out

    def pir_database_shape(self, dimensions, entry_count, entry_size_in_bytes, encoding_entry_size=False):
        """he_pir_database_shape: MulPirServer.process's plan for an IndexPirParameter -> dict with chunk_count,
        plaintexts_per_chunk, bytes_per_plaintext, entries_per_plaintext (0: split mode) and entry_size_encoding_width."""
        dims = (c_u32 * max(len(dimensions), 1))(*[int(d) for d in dimensions])
        outs = [c_size() for _ in range(5)]
        _check(load_library().he_pir_database_shape(self.h, dims, len(dimensions), int(entry_count), int(entry_size_in_bytes),
                                                    int(bool(encoding_entry_size)), *[ctypes.byref(o) for o in outs]))
        names = ("chunk_count", "plaintexts_per_chunk", "bytes_per_plaintext", "entries_per_plaintext",
                 "entry_size_encoding_width")
        return {name: int(o.value) for name, o in zip(names, outs)}

    def pir_process_database(self, entries, dimensions, entry_size_in_bytes, encoding_entry_size=False, entry_sizes=None,
                             entry_count=None, out=None, device="cuda", stream=None):
        """MulPirServer.process(database:with:using:) on the device -> (database [chunks][prod(dims)][L][N] Eval, present
        uint8 [chunks][prod(dims)]).  entries: a list of bytes-like entries, or a uint8 array / tensor
        [count][entry_size_in_bytes] padded past each entry's size (entry_sizes: their byte counts; None: all full).
        entry_count: IndexPirParameter.entryCount (None: the number given); out: (database, present) to write into."""
        import torch

        sizes = None
        if isinstance(entries, (list, tuple)):
            sizes = np.array([len(e) for e in entries], dtype=np.uint64)
            padded = np.zeros((len(entries), int(entry_size_in_bytes)), dtype=np.uint8)
            for row, entry in enumerate(entries):  # an entry too long is cut here and rejected by the size check
                data = np.frombuffer(bytes(entry), dtype=np.uint8)[:int(entry_size_in_bytes)]
                padded[row, :len(data)] = data
            entries = padded
        if entry_sizes is not None:
            sizes = np.ascontiguousarray(entry_sizes, dtype=np.uint64)
        count = int(entries.shape[0])
        if entry_count is not None and int(entry_count) != count:  # PirError.invalidDatabaseEntryCount (MulPir.swift:433-436)
            raise HeError(16, f"Invalid database: Database has {count} entries, expected {int(entry_count)}")
        if sizes is not None and len(sizes) != count:
            raise ValueError("entry_sizes must give one size per entry")
        shape = self.pir_database_shape(dimensions, count, entry_size_in_bytes, encoding_entry_size)
        chunks, per_chunk = shape["chunk_count"], shape["plaintexts_per_chunk"]
        if isinstance(entries, np.ndarray):
            entries = torch.from_numpy(np.ascontiguousarray(entries, dtype=np.uint8)).to(device)
        if entries.dtype != torch.uint8 or not entries.is_cuda or not entries.is_contiguous():
            raise ValueError("entries must be a contiguous uint8 device tensor")
        if out is None:
            database = _empty((chunks, per_chunk, self.L, self.degree), self._word, entries.device)
            present = torch.empty((chunks, per_chunk), dtype=torch.uint8, device=entries.device)
        else:
            database, present = out
            if database.numel() != chunks * per_chunk * self.L * self.degree or present.numel() != chunks * per_chunk:
                raise ValueError("out tensors do not hold the database's shape")
        dims = (c_u32 * len(dimensions))(*[int(d) for d in dimensions])
        size_ptr = sizes.ctypes.data_as(U64P) if sizes is not None else None
        _check(_entry("he_pir_process_database_device", self._word)(
            self.h, dims, len(dimensions), vp(entries.data_ptr()), size_ptr, count, int(entry_size_in_bytes),
            int(bool(encoding_entry_size)), _ptr(database, self._word), vp(present.data_ptr()), _stream(stream)))
        return database, present

    # ---- the MulPIR client: MulPirClient.generateQuery / decrypt(response:) / decryptFull on the device.  The
    # IndexPirParameter is given as its fields, as pir_database_shape takes them.
    PIR_KEY_COMPRESSION = {"none": 0, "hybrid": 1, "max": 2}

    @staticmethod
    def _pir_parameter(dimensions, entry_count, entry_size_in_bytes, encoding_entry_size, indices_count):
        dims = (c_u32 * max(len(dimensions), 1))(*[int(d) for d in dimensions])
        return (dims, len(dimensions), int(entry_count), int(entry_size_in_bytes), int(bool(encoding_entry_size)),
                int(indices_count))

    def pir_client_plan(self, dimensions, entry_count, entry_size_in_bytes, encoding_entry_size=False, indices_count=1):
        """he_pir_client_plan -> dict with expanded_query_count (S I), query_ciphertext_count (C), reply_ciphertext_count (R),
        entries_per_plaintext (per), bytes_per_plaintext and entry_size_encoding_width."""
        outs = [c_size() for _ in range(6)]
        _check(load_library().he_pir_client_plan(
            self.h, *self._pir_parameter(dimensions, entry_count, entry_size_in_bytes, encoding_entry_size, indices_count),
            *[ctypes.byref(o) for o in outs]))
        names = ("expanded_query_count", "query_ciphertext_count", "reply_ciphertext_count", "entries_per_plaintext",
                 "bytes_per_plaintext", "entry_size_encoding_width")
        return {name: int(o.value) for name, o in zip(names, outs)}

    def pir_evaluation_key_elements(self, expanded_query_count, key_compression="none"):
        """MulPir.evaluationKeyConfig's Galois elements, in the reference's order: what generate_galois_keys takes."""
        lib, strategy, count = load_library(), self.PIR_KEY_COMPRESSION[key_compression], c_size()
        _check(lib.he_pir_evaluation_key_elements(self.degree, int(expanded_query_count), strategy, None, 0, ctypes.byref(count)))
        elements = _u64([0] * max(count.value, 1))
        _check(lib.he_pir_evaluation_key_elements(self.degree, int(expanded_query_count), strategy,
                                                  elements.ctypes.data_as(U64P), count.value, None))
        return [int(e) for e in elements[:count.value]]

    def pir_generate_query_workspace_bytes(self, dimensions, entry_count, entry_size_in_bytes, encoding_entry_size=False,
                                           indices_count=1, queries=1):
        return int(load_library().he_pir_generate_query_workspace_bytes(
            self.h, self._word.bits,
            *self._pir_parameter(dimensions, entry_count, entry_size_in_bytes, encoding_entry_size, indices_count), int(queries)))

    def pir_generate_query(self, indices, dimensions, entry_count, entry_size_in_bytes, encoding_entry_size, secret_key,
                           a_seeds, error_seeds, out_of_range=None, stream=None, workspace=None):
        """MulPirClient.generateQuery(at:using:) per row of indices (int64 CUDA tensor [queries][I]); seeds uint8
        [queries][C][32] -> (ciphertexts [queries][C][2][L][N] Coeff, out_of_range int32 [1]); ciphertexts[q] is the
        query_ciphertexts of pir_compute_response_to_query."""
        import torch

        if indices.dtype != torch.int64 or not indices.is_cuda or not indices.is_contiguous() or indices.dim() != 2:
            raise ValueError("indices must be a contiguous int64 device tensor [queries][indices_count]")
        queries, count = int(indices.shape[0]), int(indices.shape[1])
        w = self._word
        plan = self.pir_client_plan(dimensions, entry_count, entry_size_in_bytes, encoding_entry_size, max(count, 1))
        out = _empty((queries, plan["query_ciphertext_count"], 2, self.L, self.degree), w, indices.device)
        if out_of_range is None:
            out_of_range = torch.zeros((1,), dtype=torch.int32, device=indices.device)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(load_library().he_pir_generate_query_device(
            self.h, w.bits, *self._pir_parameter(dimensions, entry_count, entry_size_in_bytes, encoding_entry_size, count),
            vp(indices.data_ptr()), queries, _ptr(secret_key, w), vp(a_seeds.data_ptr()), vp(error_seeds.data_ptr()),
            _ptr(out, w), vp(out_of_range.data_ptr()), ws_ptr, ws_bytes, _stream(stream)))
        return out, out_of_range

    def pir_decrypt_response_workspace_bytes(self, dimensions, entry_count, entry_size_in_bytes, encoding_entry_size=False,
                                             indices_count=1, queries=1, moduli_count=1):
        return int(load_library().he_pir_decrypt_response_workspace_bytes(
            self.h, self._word.bits,
            *self._pir_parameter(dimensions, entry_count, entry_size_in_bytes, encoding_entry_size, indices_count),
            int(moduli_count), int(queries)))

    def pir_decrypt_response(self, response, indices, dimensions, entry_count, entry_size_in_bytes, encoding_entry_size,
                             secret_key, stream=None, workspace=None):
        """MulPirClient.decrypt(response:at:using:): response [queries][I][R][2][moduli_count][N] Coeff, indices as
        pir_generate_query takes them -> (entries uint8 [queries][I][E], zeros behind each entry's size; sizes int64
        [queries][I]).  indices None: decryptFull, entries [queries][I][R bpp]."""
        import torch

        w = self._word
        if (response.dim() != 6 or response.shape[3] != 2 or response.shape[5] != self.degree
                or (indices is not None and tuple(indices.shape) != tuple(response.shape[:2]))):
            raise ValueError("expected the response as [queries][indices][R][2][moduli_count][N] and indices as [queries][indices]")
        if indices is not None and (indices.dtype != torch.int64 or not indices.is_cuda or not indices.is_contiguous()):
            raise ValueError("indices must be a contiguous int64 device tensor")
        queries, count, moduli_count = int(response.shape[0]), int(response.shape[1]), int(response.shape[4])
        plan = self.pir_client_plan(dimensions, entry_count, entry_size_in_bytes, encoding_entry_size, max(count, 1))
        if response.shape[2] != plan["reply_ciphertext_count"]:  # PirError.invalidReply
            raise HeError(16, f"Invalid reply: ciphertext count {int(response.shape[2])}, expected "
                              f"{plan['reply_ciphertext_count']}")
        stride = (int(entry_size_in_bytes) if indices is not None
                  else plan["reply_ciphertext_count"] * plan["bytes_per_plaintext"])
        entries = torch.empty((queries, count, stride), dtype=torch.uint8, device=response.device)
        sizes = torch.empty((queries, count), dtype=torch.int64, device=response.device)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(load_library().he_pir_decrypt_response_device(
            self.h, w.bits, *self._pir_parameter(dimensions, entry_count, entry_size_in_bytes, encoding_entry_size, count),
            moduli_count, _ptr(response, w), vp() if indices is None else vp(indices.data_ptr()), queries,
            _ptr(secret_key, w), vp(entries.data_ptr()), vp(sizes.data_ptr()), ws_ptr, ws_bytes, _stream(stream)))
        return entries, sizes

    # ---- the keyword PIR client: KeywordPirClient.generateQuery / decrypt(response:) / countEntriesInResponse on
    # the device.  entry_count is the table's buckets_per_table, entry_size_in_bytes the bucket row, h the hash function count;
    # keywords: a uint8 device tensor at any byte address with keyword_offsets an int64 device tensor [queries + 1].
    KEYWORD_PIR_FIND_FORMS = {None: -1, "plan": -1, "staged": 0, "direct": 1}

    @staticmethod
    def _keyword_parameter(dimensions, entry_count, entry_size_in_bytes, hash_function_count):
        dims = (c_u32 * max(len(dimensions), 1))(*[int(d) for d in dimensions])
        return dims, len(dimensions), int(entry_count), int(entry_size_in_bytes), int(hash_function_count)

    def keyword_pir_client_plan(self, dimensions, entry_count, entry_size_in_bytes, hash_function_count):
        """he_keyword_client_plan -> pir_client_plan's values (but the encoding width) and value_capacity, find_form
        ("staged" or "direct"), staged_lds_bytes and reply_bytes."""
        outs, form, more = [c_size() for _ in range(6)], ctypes.c_int(), [c_size() for _ in range(2)]
        _check(load_library().he_keyword_client_plan(
            self.h, *self._keyword_parameter(dimensions, entry_count, entry_size_in_bytes, hash_function_count),
            *[ctypes.byref(o) for o in outs], ctypes.byref(form), *[ctypes.byref(o) for o in more]))
        names = ("expanded_query_count", "query_ciphertext_count", "reply_ciphertext_count", "entries_per_plaintext",
                 "bytes_per_plaintext", "value_capacity")
        plan = {name: int(o.value) for name, o in zip(names, outs)}
        plan.update(find_form="staged" if form.value == 0 else "direct", staged_lds_bytes=int(more[0].value),
                    reply_bytes=int(more[1].value))
        return plan

    def keyword_pir_generate_query_workspace_bytes(self, dimensions, entry_count, entry_size_in_bytes, hash_function_count,
                                                   queries=1):
        return int(load_library().he_keyword_client_generate_query_workspace_bytes(
            self.h, self._word.bits,
            *self._keyword_parameter(dimensions, entry_count, entry_size_in_bytes, hash_function_count), int(queries)))

    def keyword_pir_generate_query(self, keywords, keyword_offsets, dimensions, entry_count, entry_size_in_bytes,
                                   hash_function_count, secret_key, a_seeds, error_seeds, stream=None, workspace=None):
        """KeywordPirClient.generateQuery(at:using:) per keyword; seeds uint8 [queries][C][32] -> (ciphertexts
        [queries][C][2][L][N] Coeff, the keyword hashes int64 [queries])."""
        import torch

        queries, w = keyword_offsets.numel() - 1, self._word
        plan = self.keyword_pir_client_plan(dimensions, entry_count, entry_size_in_bytes, hash_function_count)
        out = _empty((queries, plan["query_ciphertext_count"], 2, self.L, self.degree), w, keywords.device)
        hashes = torch.empty((queries,), dtype=torch.int64, device=keywords.device)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(load_library().he_keyword_client_generate_query_device(
            self.h, w.bits, *self._keyword_parameter(dimensions, entry_count, entry_size_in_bytes, hash_function_count),
            _byte_ptr(keywords), _ptr(keyword_offsets), queries, _ptr(secret_key, w), vp(a_seeds.data_ptr()),
            vp(error_seeds.data_ptr()), _ptr(out, w), _ptr(hashes), ws_ptr, ws_bytes, _stream(stream)))
        return out, hashes

    @staticmethod
    def keyword_pir_find_in_buckets(buckets, hashes, form=None, out_values=None, stream=None, workspace=None):
        """he_keyword_client_find_in_buckets_device: buckets uint8 [queries][h][E] (any byte address), hashes int64 [queries] ->
        (values uint8 [queries][value_capacity], the value and zeros behind it; sizes int64 [queries]; status int32 [queries]:
        0 nil, 1 found, 2 corruptedData).  form: None (the plan's), "staged" or "direct"."""
        import torch

        if buckets.dim() != 3 or buckets.shape[0] != hashes.numel():
            raise ValueError("expected buckets as [queries][hash_function_count][entry_size] and one hash a query")
        queries, h, size = (int(d) for d in buckets.shape)
        capacity = 0 if size < 11 else min(size - 11, 65535)
        if out_values is None:
            out_values = torch.empty((queries, capacity), dtype=torch.uint8, device=buckets.device)
        elif out_values.numel() != queries * capacity:
            raise ValueError("out_values does not hold queries * value_capacity bytes")
        sizes = torch.empty((queries,), dtype=torch.int64, device=buckets.device)
        status = torch.empty((queries,), dtype=torch.int32, device=buckets.device)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(load_library().he_keyword_client_find_in_buckets_device(
            _byte_ptr(buckets), _ptr(hashes), size, h, queries, BfvContext.KEYWORD_PIR_FIND_FORMS[form], _byte_ptr(out_values),
            _ptr(sizes), _ptr(status, WORD32), ws_ptr, ws_bytes, _stream(stream)))
        return out_values, sizes, status

    def keyword_pir_decrypt_response_workspace_bytes(self, dimensions, entry_count, entry_size_in_bytes, hash_function_count,
                                                     queries=1, moduli_count=1):
        return int(load_library().he_keyword_client_decrypt_response_workspace_bytes(
            self.h, self._word.bits,
            *self._keyword_parameter(dimensions, entry_count, entry_size_in_bytes, hash_function_count), int(moduli_count),
            int(queries)))

    def keyword_pir_decrypt_response(self, response, dimensions, entry_count, entry_size_in_bytes, secret_key, keywords=None,
                                     keyword_offsets=None, hashes=None, stream=None, workspace=None):
        """KeywordPirClient.decrypt(response:at:using:): response [queries][h][R][2][moduli_count][N] Coeff and the keywords
        (or their hashes, int64 [queries]) -> (values, sizes, status) as keyword_pir_find_in_buckets gives them."""
        import torch

        w = self._word
        if response.dim() != 6 or response.shape[3] != 2 or response.shape[5] != self.degree:
            raise ValueError("expected the response as [queries][hash_function_count][R][2][moduli_count][N]")
        if (keywords is None) == (hashes is None) or (keywords is not None and keyword_offsets is None):
            raise ValueError("give the keywords with their offsets, or their hashes")
        queries, h, moduli_count = int(response.shape[0]), int(response.shape[1]), int(response.shape[4])
        plan = self.keyword_pir_client_plan(dimensions, entry_count, entry_size_in_bytes, h)
        if response.shape[2] != plan["reply_ciphertext_count"]:  # PirError.invalidReply
            raise HeError(16, f"Invalid reply: ciphertext count {int(response.shape[2])}, expected "
                              f"{plan['reply_ciphertext_count']}")
        values = torch.empty((queries, plan["value_capacity"]), dtype=torch.uint8, device=response.device)
        sizes = torch.empty((queries,), dtype=torch.int64, device=response.device)
        status = torch.empty((queries,), dtype=torch.int32, device=response.device)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(load_library().he_keyword_client_decrypt_response_device(
            self.h, w.bits, *self._keyword_parameter(dimensions, entry_count, entry_size_in_bytes, h), moduli_count,
            _ptr(response, w), vp() if keywords is None else _byte_ptr(keywords), _opt_ptr(keyword_offsets), _opt_ptr(hashes),
            queries, _ptr(secret_key, w), vp(values.data_ptr()), _ptr(sizes), _ptr(status, WORD32), ws_ptr, ws_bytes,
            _stream(stream)))
        return values, sizes, status

    def keyword_pir_count_entries_workspace_bytes(self, dimensions, entry_count, entry_size_in_bytes, hash_function_count,
                                                  queries=1, moduli_count=1):
        return int(load_library().he_keyword_client_count_entries_workspace_bytes(
            self.h, self._word.bits,
            *self._keyword_parameter(dimensions, entry_count, entry_size_in_bytes, hash_function_count), int(moduli_count),
            int(queries)))

    def keyword_pir_count_entries(self, response, dimensions, entry_count, entry_size_in_bytes, secret_key, stream=None,
                                  workspace=None):
        """KeywordPirClient.countEntriesInResponse: response as keyword_pir_decrypt_response takes it -> int64 [queries]."""
        import torch

        w = self._word
        if response.dim() != 6 or response.shape[3] != 2 or response.shape[5] != self.degree:
            raise ValueError("expected the response as [queries][hash_function_count][R][2][moduli_count][N]")
        queries, h, moduli_count = int(response.shape[0]), int(response.shape[1]), int(response.shape[4])
        counts = torch.empty((queries,), dtype=torch.int64, device=response.device)
        ws_ptr, ws_bytes = _workspace(workspace)
        _check(load_library().he_keyword_client_count_entries_device(
            self.h, w.bits, *self._keyword_parameter(dimensions, entry_count, entry_size_in_bytes, h), moduli_count,
            _ptr(response, w), queries, _ptr(secret_key, w), _ptr(counts), ws_ptr, ws_bytes, _stream(stream)))
        return counts

    @staticmethod
    def keyword_pir_count_bucket_entries(replies, stream=None):
        """he_keyword_client_count_bucket_entries_device: the scan of countEntriesInResponse over replies uint8
        [queries][replies_per_query][reply_bytes] (any byte address) -> int64 [queries]."""
        import torch

        if replies.dim() != 3:
            raise ValueError("expected the replies as [queries][replies_per_query][reply_bytes]")
        queries, per_query, reply_bytes = (int(d) for d in replies.shape)
        counts = torch.empty((queries,), dtype=torch.int64, device=replies.device)
        _check(load_library().he_keyword_client_count_bucket_entries_device(
            vp(replies.data_ptr()) if replies.numel() else vp(), reply_bytes, per_query, queries, _ptr(counts), _stream(stream)))
        return counts

    # ---- processed-database files: ProcessedDatabase.serialize() / init(from:context:) ----
    def database_file_payload_bytes(self):
        """S: the bytes of a present plaintext behind its tag."""
        return self.ciphertext_context().serialization_byte_count(0)

    def database_file_byte_count(self, present):
        """he_pir_database_file_byte_count of a whole file with this host mask."""
        mask = np.ascontiguousarray(present, dtype=np.uint8).reshape(-1)
        out = c_size()
        _check(load_library().he_pir_database_file_byte_count(self.h, vp(mask.ctypes.data), mask.size, ctypes.byref(out)))
        return int(out.value)

    def scan_database_file(self, data):
        """he_pir_database_file_scan over the host image of a file -> dict(count, present (uint8 array), present_count,
        bytes_consumed).  Host only."""
        image = np.frombuffer(data, dtype=np.uint8)
        claimed = int.from_bytes(bytes(image[1:5]), "little") if image.size >= 5 else 0
        present = np.zeros(min(claimed, max(image.size - 5, 0)), dtype=np.uint8)  # a plaintext takes a byte at the least
        outs = [c_size() for _ in range(3)]
        _check(load_library().he_pir_database_file_scan(self.h, vp(image.ctypes.data), image.size, vp(present.ctypes.data),
                                                        present.size, *[ctypes.byref(o) for o in outs]))
        return {"count": int(outs[0].value), "present": present[:int(outs[0].value)], "present_count": int(outs[1].value),
                "bytes_consumed": int(outs[2].value)}

    def load_database_segment(self, records, present, records_bytes=None, out=None, mismatch=None, stream=None):
        """he_pir_database_load_device(_u32): records (uint8 device tensor, from the tag of the segment's first plaintext),
        present (uint8 device tensor [count]) -> database [count][L][N]; mismatch: a zeroed int32 device tensor."""
        count = present.numel()
        if out is None:
            out = _empty((count, self.L, self.degree), self._word, records.device)
        elif out.numel() != count * self.L * self.degree:
            raise ValueError("out does not hold the segment's plaintexts")
        size = records.numel() if records_bytes is None else int(records_bytes)
        _check(_entry("he_pir_database_load_device", self._word)(
            self.h, vp(records.data_ptr()), size, vp(present.data_ptr()), count, _ptr(out, self._word),
            None if mismatch is None else vp(mismatch.data_ptr()), _stream(stream)))
        return out

    def save_database_segment(self, database, present, records_bytes=None, out=None, mismatch=None, stream=None):
        """he_pir_database_save_device(_u32): tags and payloads of database [count][L][N] under present (uint8 device tensor;
        its host sum sizes `out` when that is not given) -> uint8 device tensor."""
        import torch

        count = present.numel()
        if database.numel() != count * self.L * self.degree:
            raise ValueError("database does not hold one plaintext per mask byte")
        if out is None:
            need = count + self.database_file_payload_bytes() * int((present != 0).sum().item())
            out = torch.empty(need if records_bytes is None else int(records_bytes), dtype=torch.uint8, device=database.device)
        size = out.numel() if records_bytes is None else int(records_bytes)
        _check(_entry("he_pir_database_save_device", self._word)(
            self.h, _ptr(database, self._word), vp(present.data_ptr()), count, vp(out.data_ptr()), size,
            None if mismatch is None else vp(mismatch.data_ptr()), _stream(stream)))
        return out

    def load_database_file(self, data, device="cuda", stream=None):
        """ProcessedDatabase.init(from:context:) on the device: scan on the host, upload, load -> (database [count][L][N],
        present uint8 [count]).  Trailing bytes are ignored, as the reference ignores them."""
        import torch

        scan = self.scan_database_file(data)
        image = np.frombuffer(data, dtype=np.uint8)[5:scan["bytes_consumed"]]
        records = torch.from_numpy(image.copy()).to(device)
        present = torch.from_numpy(scan["present"].copy()).to(device)
        mismatch = torch.zeros(1, dtype=torch.int32, device=device)
        database = self.load_database_segment(records, present, mismatch=mismatch, stream=stream)
        if int(mismatch.item()) != 0:  # (cannot happen after a scan of the same bytes)
            raise HeError(16, "the database file does not hold what its tags announce")
        return database, present

    def save_database_file(self, database, present, stream=None):
        """ProcessedDatabase.serialize(): the header from the host entry, the body from the device -> bytes."""
        header = (ctypes.c_uint8 * 5)()
        _check(load_library().he_pir_database_file_header(present.numel(), header))
        if present.numel() == 0:
            return bytes(header)
        body = self.save_database_segment(database.reshape(-1), present.reshape(-1), stream=stream)
        if stream is not None:
            stream.synchronize()
        return bytes(header) + body.cpu().numpy().tobytes()

    def packed_plaintext_words(self, moduli_count=None):
        return int(load_library().he_bfv_packed_plaintext_words(self.h, self._L(moduli_count)))

    def pack_plaintexts(self, plaintexts_eval, moduli_count=None, stream=None):
        """[...][L][N] Eval plaintexts -> [count * words + 1] packed words (one word of padding: the kernels read 8 bytes
        past the last field)."""
        import torch

        L = self._L(moduli_count)
        count = plaintexts_eval.numel() // (L * self.degree)
        words = self.packed_plaintext_words(L)
        out = torch.zeros(count * words + 1, dtype=torch.int64, device=plaintexts_eval.device)
        _check(load_library().he_bfv_pack_plaintexts_device(self.h, L, _ptr(plaintexts_eval), count, _ptr(out),
                                                            _stream(stream)))
        return out

    def inner_product_plain_packed(self, cts, packed_pts, present_device=None, poly_count=2, columns=1, moduli_count=None,
                                   stream=None):
        L = self._L(moduli_count)
        count = cts.numel() // (poly_count * L * self.degree)
        out = _empty((columns, poly_count, L, self.degree), WORD64, cts.device)
        mask = vp() if present_device is None else vp(present_device.data_ptr())
        _check(load_library().he_bfv_inner_product_plain_packed_device(self.h, L, poly_count, _ptr(cts), _ptr(packed_pts),
                                                                       mask, count, columns, _ptr(out), _stream(stream)))
        return out

    def pir_compute_response_packed(self, dimensions, dim0_query_eval, remaining_query, packed_database, chunk_count,
                                    present_device=None, relinearization_key=None, stream=None):
        dims = (c_u32 * len(dimensions))(*[int(d) for d in dimensions])
        out = _empty((chunk_count, 2, 1, self.degree), WORD64, dim0_query_eval.device)
        rest = _opt_ptr(remaining_query)
        rest_count = 0 if remaining_query is None else remaining_query.numel() // (2 * self.L * self.degree)
        key = _opt_ptr(relinearization_key)
        mask = vp() if present_device is None else vp(present_device.data_ptr())
        _check(load_library().he_pir_compute_response_packed_device(self.h, dims, len(dimensions), _ptr(dim0_query_eval),
                                                                    rest, rest_count, _ptr(packed_database), mask,
                                                                    chunk_count, key, _ptr(out), _stream(stream)))
        return out

    def inner_product(self, lhs, rhs, moduli_count=None, stream=None):
        L, w = self._L(moduli_count), self._word
        count = lhs.numel() // (2 * L * self.degree)
        out = _empty((3, L, self.degree), w, lhs.device)
        _check(_entry("he_bfv_inner_product_device", w)(
            self.h, L, _ptr(lhs, w), _ptr(rhs, w), count, _ptr(out, w), vp(), 0, _stream(stream)))
        return out

    def inner_product_shared(self, lhs, rhs, moduli_count=None, stream=None):
        """rhs [items][count][2][L][N]: `items` inner products with the same left vector -> [items][3][L][N]."""
        L, w = self._L(moduli_count), self._word
        count = lhs.numel() // (2 * L * self.degree)
        items = rhs.numel() // (count * 2 * L * self.degree)
        out = _empty((items, 3, L, self.degree), w, lhs.device)
        _check(_entry("he_bfv_inner_product_shared_device", w)(
            self.h, L, _ptr(lhs, w), _ptr(rhs, w), count, items, _ptr(out, w), _stream(stream)))
        return out


class BfvContext32(BfvContext):
    """Context<Bfv<UInt32>> on PACKED [UInt32] slabs (int32 tensors): the `_u32` entry points of include/he_amd.h.
    Same shapes as BfvContext's methods; nothing is widened in memory."""

    def __init__(self, degree, plaintext_modulus, coefficient_moduli, host_only=False):
        super().__init__(degree, plaintext_modulus, coefficient_moduli, host_only=host_only, word_bits=32)

    _word = WORD32


def skip_lsbs_for_decryption(degree, q0, plaintext_modulus, moduli_count=1):
    """Bfv.skipLSBsForDecryption -> [poly0, poly1].  Host only."""
    out = (ctypes.c_int * 2)()
    _check(load_library().he_bfv_skip_lsbs_for_decryption(int(degree), int(q0), int(plaintext_modulus), int(moduli_count),
                                                          out))
    return [out[0], out[1]]


def simple_pir_shape(plaintext_bits, ciphertext_bits, lattice_dimension, entry_count, entry_size_in_bytes, word_bits=64):
    """he_simple_pir_shape: SimplePirServerProtocol.computingParams, process's padded column size and SimplePirContext's
    modulus -> dict.  Host only."""
    sizes = [c_size(0) for _ in range(6)]
    modulus, element_bytes = c_u64(0), c_u32(0)
    _check(load_library().he_simple_pir_shape(int(plaintext_bits), int(ciphertext_bits), int(lattice_dimension), int(word_bits),
                                              int(entry_count), int(entry_size_in_bytes), *[ctypes.byref(v) for v in sizes],
                                              ctypes.byref(modulus), ctypes.byref(element_bytes)))
    names = ("entry_size_in_scalar", "entries_per_column", "chunks_per_entry", "database_columns", "column_size", "a_poly_count")
    out = {name: v.value for name, v in zip(names, sizes)}
    out.update(modulus=modulus.value, element_bytes=element_bytes.value, plaintext_bits=int(plaintext_bits),
               ciphertext_bits=int(ciphertext_bits), lattice_dimension=int(lattice_dimension),
               entry_size_in_bytes=int(entry_size_in_bytes), entry_count=int(entry_count))
    return out


def simple_pir_batch_plan(plaintext_bits, ciphertext_bits, database_columns, query_count, word_bits=64):
    """he_simple_pir_batch_response_plan: what SimplePirServer.compute_response_batch does for a shape -> dict.  Host only."""
    words = [c_u32(0) for _ in range(4)]
    sizes = [c_size(0) for _ in range(2)]
    _check(load_library().he_simple_pir_batch_response_plan(int(plaintext_bits), int(ciphertext_bits), int(word_bits),
                                                            int(database_columns), int(query_count),
                                                            *[ctypes.byref(v) for v in words + sizes]))
    names = ("matrix_path", "database_limbs", "request_limbs", "requests_per_pass", "fold_columns", "workspace_bytes")
    return {name: v.value for name, v in zip(names, words + sizes)}


_SIMPLE_PIR_ELEMENT_DTYPES = {1: "uint8", 2: "int16", 4: "int32", 8: "int64"}


class SimplePirServer:
    """SimplePirServer<UInt64> (PrivateInformationRetrieval/SimplePir/SimplePir+Server.swift) on the device: `database` is a
    torch tensor [column_size][database_columns] of element_bytes-wide elements, `hint` [column_size][lattice_dimension]
    words mod params["modulus"], requests and responses torch tensors of words (int64 storage; int32 in SimplePirServer32)."""

    _word = WORD64
    word_bits = _word.bits

    def __init__(self, database, hint, params, _handle=None):
        self.database, self.hint, self.params = database, hint, params
        self.h = _handle  # he_simple_pir_context of a server made by process(); None for one made from a wide image

    def __del__(self):
        if getattr(self, "h", None):
            load_library().he_simple_pir_context_destroy(self.h)
            self.h = None

    @classmethod
    def process(cls, entries, plaintext_bits, ciphertext_bits, lattice_dimension, seed, stream=None):
        """SimplePirServerProtocol.process: entries a uint8 CUDA tensor [entry_count][entry_size_in_bytes], seed 32 bytes
        (bytes-like, uploaded here, or a uint8 CUDA tensor).  Creates the server's he_simple_pir_context (that synchronises:
        tables are uploaded), which the server keeps until it is collected; the database and hint are then enqueued on
        `stream` and the call returns with that work in flight."""
        if entries.dim() != 2:
            raise ValueError("expected entries [entry_count][entry_size_in_bytes]")
        entry_count, entry_size = entries.shape
        params = simple_pir_shape(plaintext_bits, ciphertext_bits, lattice_dimension, entry_count, entry_size, cls.word_bits)
        handle = vp()
        _check(load_library().he_simple_pir_context_create(int(plaintext_bits), int(ciphertext_bits), int(lattice_dimension),
                                                           cls.word_bits, entry_count, entry_size, ctypes.byref(handle)))
        server = cls(None, None, params, handle)
        return server.reprocess(entries, seed, stream)

    def reprocess(self, entries, seed, stream=None, out=None):
        """process again with the server's context (entries of the same shape; another seed or other bytes): enqueue-only
        when the seed is a CUDA tensor.  out = (database, hint) tensors to write into instead of fresh ones."""
        import torch

        if self.h is None:
            raise ValueError("this server was not made by process()")
        params = self.params
        if (not entries.is_cuda or not entries.is_contiguous() or entries.element_size() != 1
                or tuple(entries.shape) != (params["entry_count"], params["entry_size_in_bytes"])):
            raise ValueError("expected a contiguous CUDA uint8 tensor [entry_count][entry_size_in_bytes]")
        if not torch.is_tensor(seed):
            seed = torch.from_numpy(np.frombuffer(bytes(seed), dtype=np.uint8).copy()).to(entries.device)
        if seed.numel() != 32 or seed.element_size() != 1 or not seed.is_cuda:
            raise ValueError("expected a 32-byte seed")
        if out is None:
            database = torch.empty((params["column_size"], params["database_columns"]), device=entries.device,
                                   dtype=getattr(torch, _SIMPLE_PIR_ELEMENT_DTYPES[params["element_bytes"]]))
            hint = _empty((params["column_size"], params["lattice_dimension"]), self._word, entries.device)
        else:
            database, hint = out
        _check(_entry("he_simple_pir_process_database_device", self._word)(
            self.h, vp(entries.data_ptr()), vp(seed.data_ptr()), vp(database.data_ptr()), vp(hint.data_ptr()), _stream(stream)))
        self.database, self.hint = database, hint
        return self

    @classmethod
    def from_wide(cls, wide, hint, params, stream=None):
        """init(processedDatabase:hint:params:) from the reference's wide image [column_size][database_columns] of words."""
        import torch

        database = torch.empty(tuple(wide.shape), device=wide.device,
                               dtype=getattr(torch, _SIMPLE_PIR_ELEMENT_DTYPES[params["element_bytes"]]))
        _check(_entry("he_simple_pir_pack_database_device", cls._word)(
            params["plaintext_bits"], _ptr(wide, cls._word), vp(database.data_ptr()), wide.numel(), _stream(stream)))
        return cls(database, hint, params)

    def wide_database(self, stream=None):
        """The database as the reference stores it: one word per element."""
        wide = _empty(tuple(self.database.shape), self._word, self.database.device)
        _check(_entry("he_simple_pir_unpack_database_device", self._word)(
            self.params["plaintext_bits"], vp(self.database.data_ptr()), vp(wide.data_ptr()), wide.numel(), _stream(stream)))
        return wide

    def compute_response(self, requests, stream=None):
        """computeResponse(to:): requests [query_count][database_columns] -> responses [query_count][column_size]."""
        if requests.dim() != 2 or requests.shape[1] != self.params["database_columns"]:
            raise ValueError("expected requests [query_count][database_columns]")
        responses = _empty((requests.shape[0], self.params["column_size"]), self._word, requests.device)
        _check(_entry("he_simple_pir_compute_response_device", self._word)(
            self.params["plaintext_bits"], self.params["ciphertext_bits"], vp(self.database.data_ptr()),
            self.params["column_size"], self.params["database_columns"], _ptr(requests, self._word), requests.shape[0],
            vp(responses.data_ptr()), _stream(stream)))
        return responses

    def compute_response_batch(self, requests, stream=None):
        """computeResponse(to:) for large batches: the words of compute_response, formed on the int8 matrix cores where
        simple_pir_batch_plan says so (elements must be below 2^plaintext_bits, as process and from_wide leave them)."""
        if requests.dim() != 2 or requests.shape[1] != self.params["database_columns"]:
            raise ValueError("expected requests [query_count][database_columns]")
        responses = _empty((requests.shape[0], self.params["column_size"]), self._word, requests.device)
        _check(_entry("he_simple_pir_compute_response_batch_device", self._word)(
            self.params["plaintext_bits"], self.params["ciphertext_bits"], vp(self.database.data_ptr()),
            self.params["column_size"], self.params["database_columns"], _ptr(requests, self._word), requests.shape[0],
            vp(responses.data_ptr()), _stream(stream)))
        return responses

    def batch_plan(self, query_count):
        return simple_pir_batch_plan(self.params["plaintext_bits"], self.params["ciphertext_bits"],
                                     self.params["database_columns"], query_count, self.word_bits)


class SimplePirServer32(SimplePirServer):
    """SimplePirServer<UInt32>: 4-byte request / response / hint words."""

    _word = WORD32
    word_bits = _word.bits


SIMPLE_PIR_ERROR_STD_DEVS = {"stdDev32": 0, "stdDev64": 1}  # ErrorStdDev (HE_SIMPLE_PIR_ERROR_*)
_SIMPLE_PIR_CLIENT_OPS = {"a_polynomials": 0, "encrypt_zero": 1, "secret_times_hint": 2, "precompute": 3, "decrypt_responses": 4}


def simple_pir_client_plan(plaintext_bits, ciphertext_bits, lattice_dimension, entry_count, entry_size_in_bytes,
                           error_std_dev="stdDev32", batch=1, word_bits=64):
    """he_simple_pir_client_plan: what the SimplePirClient entries do for a shape and a batch -> dict.  Host only."""
    sizes = {name: c_size(0) for name in (
        "chunk_size", "query_words", "result_words", "row_block", "hint_product_lds_bytes", "a_polynomials_workspace_bytes",
        "encrypt_zero_workspace_bytes", "secret_times_hint_workspace_bytes", "precompute_workspace_bytes",
        "decrypt_responses_workspace_bytes")}
    stream_bytes, rows_per_pass, fold_terms = c_u32(0), c_u32(0), c_u64(0)
    ref = ctypes.byref
    _check(load_library().he_simple_pir_client_plan(
        int(plaintext_bits), int(ciphertext_bits), int(lattice_dimension), int(word_bits), int(entry_count),
        int(entry_size_in_bytes), SIMPLE_PIR_ERROR_STD_DEVS.get(error_std_dev, error_std_dev), int(batch),
        ref(sizes["chunk_size"]), ref(sizes["query_words"]), ref(sizes["result_words"]), ref(stream_bytes), ref(rows_per_pass),
        ref(fold_terms), ref(sizes["row_block"]), ref(sizes["hint_product_lds_bytes"]),
        ref(sizes["a_polynomials_workspace_bytes"]), ref(sizes["encrypt_zero_workspace_bytes"]),
        ref(sizes["secret_times_hint_workspace_bytes"]), ref(sizes["precompute_workspace_bytes"]),
        ref(sizes["decrypt_responses_workspace_bytes"])))
    out = {name: v.value for name, v in sizes.items()}
    out.update(error_stream_bytes=stream_bytes.value, secret_rows_per_pass=rows_per_pass.value, fold_terms=fold_terms.value)
    return out


class SimplePirClient:
    """SimplePirClient / PrecomputedQueries (PrivateInformationRetrieval/SimplePir/SimplePir+Client.swift,
    SimplePir+Precompute.swift) on the device, for batches of B independent queries: made from a server's params, hint and
    seed.  Slabs are torch tensors of words of `word_bits` (int64 / int32 storage); seeds uint8 CUDA tensors [..][32].  Every
    method allocates its workspace unless one is passed (a uint8 CUDA tensor, 16-byte aligned) and is enqueue-only."""

    def __init__(self, params, hint, seed, word_bits=64, error_std_dev="stdDev32"):
        import torch

        self._word = _word_of(word_bits)
        self.word_bits = self._word.bits
        self.params, self.hint = params, hint
        self.error_std_dev = SIMPLE_PIR_ERROR_STD_DEVS[error_std_dev]
        if not torch.is_tensor(seed):
            seed = torch.from_numpy(np.frombuffer(bytes(seed), dtype=np.uint8).copy()).to(hint.device)
        self.seed = seed
        self.h = vp()
        _check(load_library().he_simple_pir_context_create(
            params["plaintext_bits"], params["ciphertext_bits"], params["lattice_dimension"], self.word_bits,
            params["entry_count"], params["entry_size_in_bytes"], ctypes.byref(self.h)))
        self._a = None

    def __del__(self):
        if getattr(self, "h", None):
            load_library().he_simple_pir_context_destroy(self.h)
            self.h = None

    def plan(self, batch=1):
        p = self.params
        return simple_pir_client_plan(p["plaintext_bits"], p["ciphertext_bits"], p["lattice_dimension"], p["entry_count"],
                                      p["entry_size_in_bytes"], self.error_std_dev, batch, self.word_bits)

    def workspace_bytes(self, operation, count=1):
        return load_library().he_simple_pir_client_workspace_bytes(self.h, _SIMPLE_PIR_CLIENT_OPS[operation], self.error_std_dev,
                                                                   int(count))

    def _scratch(self, operation, count, workspace):
        import torch

        if workspace is None:
            workspace = torch.empty(max(self.workspace_bytes(operation, count), 16), dtype=torch.uint8, device=self.hint.device)
        return _workspace(workspace)

    def a_polynomials(self, stream=None, workspace=None):
        """generateAPolynomials + convertToEvalFormat -> [a_poly_count][N], computed once and kept."""
        if self._a is None:
            out = _empty((self.params["a_poly_count"], self.params["lattice_dimension"]), self._word, self.hint.device)
            _check(load_library().he_simple_pir_a_polynomials_device(
                self.h, self.word_bits, vp(self.seed.data_ptr()), vp(out.data_ptr()), *self._scratch("a_polynomials", 1, workspace),
                _stream(stream)))
            self._a = out
        return self._a

    def _shape(self, batch, width):
        return (batch, self.params["chunks_per_entry"], width)

    def encrypt_zero(self, secrets, error_seeds, stream=None, workspace=None):
        """SimplePirContext.encryptZero: secrets [B][chunks][N] Coeff ternary, error_seeds [B][32] -> queries [B][chunks][D]."""
        batch = secrets.shape[0]
        queries = _empty(self._shape(batch, self.params["database_columns"]), self._word, secrets.device)
        _check(load_library().he_simple_pir_encrypt_zero_device(
            self.h, self.word_bits, self.error_std_dev, _ptr(self.a_polynomials(stream), self._word), _ptr(secrets, self._word),
            vp(error_seeds.data_ptr()), vp(queries.data_ptr()), batch, *self._scratch("encrypt_zero", batch, workspace),
            _stream(stream)))
        return queries

    def secret_times_hint(self, secrets, hint=None, stream=None, workspace=None):
        """secretMatrix.multiply(transposing: hint, modulus: p): secrets [R][N] ternary -> [R][column_size]."""
        hint = self.hint if hint is None else hint
        rows = secrets.shape[0]
        results = _empty((rows, hint.shape[0]), self._word, secrets.device)
        _check(load_library().he_simple_pir_secret_times_hint_device(
            self.h, self.word_bits, _ptr(secrets, self._word), rows, vp(hint.data_ptr()), hint.shape[0], vp(results.data_ptr()),
            *self._scratch("secret_times_hint", rows, workspace), _stream(stream)))
        return results

    def precompute(self, secret_seeds, error_seeds, stream=None, workspace=None):
        """PrecomputedQueries.WithoutIndices.init for B queries: secret_seeds [B][chunks][32], error_seeds [B][32] ->
        (queries [B][chunks][D], results_without_response [B][chunks][column_size])."""
        batch = error_seeds.shape[0]
        queries = _empty(self._shape(batch, self.params["database_columns"]), self._word, error_seeds.device)
        results = _empty(self._shape(batch, self.params["column_size"]), self._word, error_seeds.device)
        _check(load_library().he_simple_pir_precompute_queries_device(
            self.h, self.word_bits, self.error_std_dev, _ptr(self.a_polynomials(stream), self._word), _ptr(self.hint, self._word),
            vp(secret_seeds.data_ptr()), vp(error_seeds.data_ptr()), vp(queries.data_ptr()), vp(results.data_ptr()), batch,
            *self._scratch("precompute", batch, workspace), _stream(stream)))
        return queries, results

    def add_indices(self, queries, indices, stream=None):
        """WithoutIndices.add(index:) in place: indices an int64 CUDA tensor [B] -> flags [B] (1: index out of range)."""
        import torch

        flags = torch.empty(queries.shape[0], dtype=torch.int32, device=queries.device)
        _check(load_library().he_simple_pir_add_indices_device(
            self.h, self.word_bits, _ptr(queries, self._word), _ptr(indices, WORD64), vp(flags.data_ptr()), queries.shape[0],
            _stream(stream)))
        return flags

    def decrypt(self, responses, results, indices, stream=None, workspace=None):
        """prepareResponse + integrate + decrypt: responses, results [B][chunks][column_size] -> (entries uint8
        [B][entry_size_in_bytes], flags [B])."""
        import torch

        batch = responses.shape[0]
        entries = torch.empty((batch, self.params["entry_size_in_bytes"]), dtype=torch.uint8, device=responses.device)
        flags = torch.empty(batch, dtype=torch.int32, device=responses.device)
        _check(load_library().he_simple_pir_decrypt_responses_device(
            self.h, self.word_bits, _ptr(responses, self._word), _ptr(results, self._word), _ptr(indices, WORD64),
            vp(entries.data_ptr()), vp(flags.data_ptr()), batch, *self._scratch("decrypt_responses", batch, workspace),
            _stream(stream)))
        return entries, flags


SIMPLE_PIR_SHARD_FORMS = {0: "none", 1: "byte", 2: "word", 3: "wide"}  # HE_SIMPLE_PIR_SHARD_FORM_*


def simple_pir_shard_plan(value_offsets, shard_count, chunk_size, shards_address=0):
    """he_simple_pir_shard_plan: what DatabaseMap.shardDatabase does for the values whose HOST offsets are value_offsets
    [count + 1] -> dict.  shards_address: where the shard slab will lie (its low four bits decide the form).  Host only."""
    offsets = np.ascontiguousarray(np.asarray(value_offsets, dtype=np.uint64))
    if offsets.ndim != 1 or offsets.size < 1:
        raise ValueError("count + 1 offsets")
    total, largest, per_shard, scratch = c_u64(0), c_u64(0), c_u64(0), c_size(0)
    form, tile, tiles, workgroups = c_u32(0), c_u32(0), c_size(0), c_size(0)
    ref = ctypes.byref
    _check(load_library().he_simple_pir_shard_plan(
        offsets.ctypes.data_as(U64P), offsets.size - 1, int(shard_count), int(chunk_size), int(shards_address), ref(total),
        ref(largest), ref(per_shard), ref(form), ref(tile), ref(tiles), ref(workgroups), ref(scratch)))
    return {"total_chunks": total.value, "maximum_chunk_count": largest.value, "chunks_per_shard": per_shard.value,
            "scatter_form": SIMPLE_PIR_SHARD_FORMS[form.value], "map_tile_entries": tile.value, "map_tiles": tiles.value,
            "count_workgroups": workgroups.value, "scratch_bytes": scratch.value}


class SimplePirShardMap:
    """DatabaseMap + ShardMap (PrivateInformationRetrieval/SimplePir/DatabaseMap.swift, SimplePir+Shards.swift:18-45) with the
    chunk locations on the device: value_offsets and chunk_starts int64 [count + 1], chunk_shard / chunk_index / row_chunk int32
    [total_chunks], shard_row_starts int64 [S + 1].  shard_count is ShardMap.shardCount -- the shards that received a chunk,
    not the S the database was split into (requested_shard_count) -- and chunks_per_shard divides by it, as the reference does.
    positions: the host dictionary originalIndex -> position in the entry list; of duplicate indices the last stays."""

    def __init__(self, arrays, requested_shard_count, chunk_size, plan, shard_rows, original_indices=None):
        self.value_offsets, self.chunk_starts, self.chunk_shard, self.chunk_index, self.shard_row_starts, self.row_chunk = arrays
        self.requested_shard_count, self.chunk_size = int(requested_shard_count), int(chunk_size)
        self.count = self.value_offsets.numel() - 1
        self.total_chunks = plan["total_chunks"]
        self.maximum_chunk_count = plan["maximum_chunk_count"]
        self.shard_rows = [int(rows) for rows in shard_rows]
        self.shard_count = sum(1 for rows in self.shard_rows if rows != 0)
        self.chunks_per_shard = -(-self.maximum_chunk_count // self.shard_count) if self.shard_count else 0
        indices = range(self.count) if original_indices is None else original_indices
        self.positions = {int(original): position for position, original in enumerate(indices)}
        if original_indices is not None and len(original_indices) != self.count:
            raise ValueError("one original index per entry")

    def position_of(self, original_index):
        """the position of an original index in the entry list; `count` (no such entry) for one the map does not hold"""
        return self.positions.get(int(original_index), self.count)


class SimplePirDatabaseMap:
    """DatabaseMap.shardDatabase (DatabaseMap.swift:82-110) on the device."""

    @staticmethod
    def shard_database(values, value_offsets, orders, shard_count, chunk_size=None, original_indices=None, stream=None,
                       mismatch=None):
        """values: a uint8 CUDA tensor (value e is values[value_offsets[e] : value_offsets[e + 1]], any address);
        value_offsets: HOST [count + 1]; orders: uint8 [count][shard_count], each row the entry's order of the shards (the
        reference's randomShards; HOST or CUDA).  chunk_size None: ceil(largest value / shard_count), as
        SimplePIRProcessDatabase computes it (main.swift:204).  -> (SimplePirShardMap, [shard_count] uint8 views
        [rows_s][chunk_size] of one slab, each the `entries` of SimplePirServer.process).  Reads the shard row counts back (the
        views need them): synchronises."""
        import torch

        if stream is not None:  # uploads, allocations and the read-back follow the caller's stream
            with torch.cuda.stream(stream):
                return SimplePirDatabaseMap.shard_database(values, value_offsets, orders, shard_count, chunk_size,
                                                           original_indices, None, mismatch)
        offsets = np.ascontiguousarray(np.asarray(value_offsets, dtype=np.uint64))
        count, shard_count = offsets.size - 1, int(shard_count)
        if chunk_size is None:
            largest = int(np.max(np.diff(offsets.astype(np.int64)))) if count else 0
            chunk_size = max(-(-largest // shard_count), 1) if shard_count else 0
        device = values.device
        plan = simple_pir_shard_plan(offsets, shard_count, chunk_size)
        total = plan["total_chunks"]
        slab = torch.empty((total * chunk_size,), dtype=torch.uint8, device=device)
        if not torch.is_tensor(orders):
            orders = torch.from_numpy(np.ascontiguousarray(np.asarray(orders, dtype=np.uint8)))
        orders = orders.to(device)
        if orders.numel() != count * shard_count:
            raise ValueError("expected orders [count][shard_count]")
        offsets_device = torch.from_numpy(offsets.view(np.int64)).to(device)
        words = lambda n, dtype: torch.empty((n,), dtype=dtype, device=device)  # noqa: E731
        chunk_starts, row_starts = words(count + 1, torch.int64), words(shard_count + 1, torch.int64)
        chunk_shard, chunk_index, row_chunk = (words(total, torch.int32) for _ in range(3))
        lib = load_library()
        _check(lib.he_simple_pir_shard_map_device(
            _ptr(offsets_device), _byte_ptr(orders), count, shard_count, int(chunk_size), total, _ptr(chunk_starts),
            _ptr(chunk_shard, WORD32), _ptr(chunk_index, WORD32), _ptr(row_starts), _ptr(row_chunk, WORD32),
            _opt_ptr(mismatch, WORD32), _stream(stream)))
        _check(lib.he_simple_pir_shard_scatter_device(
            _byte_ptr(values), values.numel(), _ptr(offsets_device), count, int(chunk_size), total, _ptr(chunk_starts),
            _ptr(row_chunk, WORD32), _byte_ptr(slab), _stream(stream)))
        starts =[int(v) for v in row_starts.cpu().tolist()]
        bounded = [min(max(v, 0), total) for v in starts]  # (a mismatch leaves them unusable: the views stay inside the slab)
        shards = [slab[bounded[s] * chunk_size: max(bounded[s + 1], bounded[s]) * chunk_size].view(-1, int(chunk_size))
                  for s in range(shard_count)]
        shard_map = SimplePirShardMap((offsets_device, chunk_starts, chunk_shard, chunk_index, row_starts, row_chunk), shard_count,
                                      chunk_size, plan, [len(shard) for shard in shards], original_indices)
        shard_map.scatter_form = simple_pir_shard_plan(offsets, shard_count, chunk_size, slab.data_ptr())["scatter_form"]
        return shard_map, shards


class SimplePirClientForAllShards:
    """SimplePirClientForAllShards (SimplePir+Shards.swift:47-173) for batches of B lookups: the index lists of query(for:) and
    the assembly of decrypt, around per-shard SimplePirClient objects (shard s's client was made from the params and hint of
    the server that processed shard s)."""

    def __init__(self, shard_map, clients):
        if shard_map.shard_count != len(clients):  # (:65-69)
            raise ValueError(f"Mismatching shard count {shard_map.shard_count} and number of clients {len(clients)}")
        if shard_map.shard_count != shard_map.requested_shard_count:
            raise ValueError("a shard without a chunk has no database to query")
        self.shard_map, self.clients = shard_map, list(clients)

    @property
    def queries_per_shard(self):
        return self.shard_map.chunks_per_shard

    def _positions(self, original_indices):
        import torch

        m = self.shard_map
        positions = np.array([m.position_of(index) for index in original_indices], dtype=np.int64)
        return torch.from_numpy(positions).to(m.chunk_starts.device)

    def query_indices(self, original_indices, stream=None):
        """query(for:) up to add(index:) -> (indices int64 [S][B][chunks_per_shard], found int32 [B]); indices[s].reshape(-1) is
        the `indices` of clients[s].add_indices for B x chunks_per_shard queries."""
        import torch

        m = self.shard_map
        positions = self._positions(original_indices)
        batch = positions.numel()
        indices = torch.empty((m.requested_shard_count, batch, m.chunks_per_shard), dtype=torch.int64, device=positions.device)
        found = torch.empty((batch,), dtype=torch.int32, device=positions.device)
        _check(load_library().he_simple_pir_shard_query_indices_device(
            _ptr(positions), batch, m.count, m.requested_shard_count, m.total_chunks, m.maximum_chunk_count, m.chunks_per_shard,
            _ptr(m.chunk_starts), _ptr(m.chunk_shard, WORD32), _ptr(m.chunk_index, WORD32), _ptr(indices),
            _ptr(found, WORD32), _stream(stream)))
        return indices, found

    def assemble(self, chunks, indices, original_indices, stream=None):
        """decrypt after the per-shard decryptions: chunks uint8 [S][B][chunks_per_shard][chunk_size], indices as
        query_indices returned them -> (entries uint8 [B][maximum_chunk_count * chunk_size], sizes int64 [B], found int32 [B]);
        entry b is entries[b, :sizes[b]] where found[b] is 1."""
        import torch

        m = self.shard_map
        positions = self._positions(original_indices)
        batch = positions.numel()
        if tuple(chunks.shape) != (m.requested_shard_count, batch, m.chunks_per_shard, m.chunk_size):
            raise ValueError("expected chunks [shard_count][B][chunks_per_shard][chunk_size]")
        entries = torch.empty((batch, m.maximum_chunk_count * m.chunk_size), dtype=torch.uint8, device=positions.device)
        sizes = torch.empty((batch,), dtype=torch.int64, device=positions.device)
        found = torch.empty((batch,), dtype=torch.int32, device=positions.device)
        _check(load_library().he_simple_pir_shard_assemble_device(
            _byte_ptr(chunks), _ptr(indices), _ptr(positions), batch, _ptr(m.value_offsets), m.count, m.requested_shard_count,
            m.chunk_size, m.total_chunks, m.maximum_chunk_count, m.chunks_per_shard, _ptr(m.chunk_starts),
            _ptr(m.chunk_shard, WORD32), _ptr(m.chunk_index, WORD32), _byte_ptr(entries), _ptr(sizes), _ptr(found, WORD32),
            _stream(stream)))
        return entries, sizes, found


PNNS_PACKINGS = {"denseColumn": 0, "denseRow": 1, "diagonal": 2}  # MatrixPacking's case order (HE_PNNS_PACKING_*)


class PnnsPackStep(ctypes.Structure):
    """he_pnns_pack_step: `count` rotations by `step` columns."""

    _fields_ = [("step", ctypes.c_int64), ("count", ctypes.c_uint32)]


class PnnsContext:
    """he_pnns_context: the SIMD encoding side of a BfvContext / BfvContext32 (plaintextContext over [t] and
    simdEncodingMatrix on the device) and the PNNS server database built with it (PrivateNearestNeighborSearch/
    ProcessedDatabase.swift:194-229).  Borrows `bfv`, which it keeps alive."""

    def __init__(self, bfv):
        lib = load_library()
        self.bfv = bfv
        self._word = _word_of(bfv.word_bits)  # Bfv<UInt32>: packed 4-byte words, as BfvContext32 lays its slabs out
        h = vp()
        _check(_entry("he_pnns_context_create", self._word)(bfv.h, ctypes.byref(h)))
        self.h = h

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.he_pnns_context_destroy(self.h)
            self.h = None

    def matrix_shape(self, row_count, column_count, packing="diagonal", baby_step=0):
        """he_pnns_matrix_shape: PlaintextMatrix.plaintextCount and BabyStepGiantStep.init -> dict with plaintext_count,
        baby_step and giant_step.  packing: "denseColumn", "denseRow", "diagonal" or the HE_PNNS_PACKING_* number."""
        count, baby, giant = c_size(), c_u32(), c_u32()
        _check(load_library().he_pnns_matrix_shape(self.h, int(row_count), int(column_count),
                                                   int(PNNS_PACKINGS.get(packing, packing)), int(baby_step),
                                                   ctypes.byref(count), ctypes.byref(baby), ctypes.byref(giant)))
        return {"plaintext_count": int(count.value), "baby_step": int(baby.value), "giant_step": int(giant.value)}

    def quantize_rows(self, vectors, scaling_factor, stream=None):
        """Array2d<Float>.normalizedScaledAndRounded: float32 CUDA tensor [rows][cols] -> int64 tensor [rows][cols]."""
        import torch

        if vectors.dtype != torch.float32 or not vectors.is_cuda or not vectors.is_contiguous() or vectors.dim() != 2:
            raise ValueError("vectors must be a contiguous float32 device tensor [rows][cols]")
        out = torch.empty(vectors.shape, dtype=torch.int64, device=vectors.device)
        _check(load_library().he_pnns_quantize_rows_device(vp(vectors.data_ptr()), vectors.shape[0], vectors.shape[1],
                                                           float(scaling_factor), vp(out.data_ptr()), _stream(stream)))
        return out

    def diagonal_matrix(self, signed_values, baby_step=0, reduce=False, moduli_count=None, stream=None):
        """PlaintextMatrix(.diagonal, signedValues:reduce:).convertToEvalFormat(moduliCount:): int64 CUDA tensor [rows][cols]
        -> (matrix [plaintext_count][moduli_count][N] Eval words, int64 storage or int32 for a BfvContext32; out_of_range, a
        one-word int32 device tensor: 1 when reduce is off and a value was outside the centred range of t)."""
        import torch

        if (signed_values.dtype != torch.int64 or not signed_values.is_cuda or not signed_values.is_contiguous()
                or signed_values.dim() != 2):
            raise ValueError("signed_values must be a contiguous int64 device tensor [rows][cols]")
        rows, cols = signed_values.shape
        L = self.bfv._L(moduli_count)
        count = self.matrix_shape(rows, cols, "diagonal", baby_step)["plaintext_count"]
        # (a fill on the caller's stream, ahead of the build that may set the word)
        with torch.cuda.stream(stream) if stream is not None else _no_stream():
            matrix = _empty((count, L, self.bfv.degree), self._word, signed_values.device)
            out_of_range = torch.zeros(1, dtype=torch.int32, device=signed_values.device)
        _check(_entry("he_pnns_diagonal_matrix_device", self._word)(
            self.h, vp(signed_values.data_ptr()), rows, cols, int(baby_step), int(bool(reduce)), L, vp(matrix.data_ptr()),
            vp(out_of_range.data_ptr()), _stream(stream)))
        return matrix, out_of_range

    def process_database(self, vectors, scaling_factor, baby_step=0, reduce=False, moduli_count=None, stream=None):
        """Database.process for this context: quantize_rows, then diagonal_matrix -> (matrix, out_of_range)."""
        import torch

        with torch.cuda.stream(stream) if stream is not None else _no_stream():
            rounded = self.quantize_rows(vectors, scaling_factor, stream=stream)
        return self.diagonal_matrix(rounded, baby_step=baby_step, reduce=reduce, moduli_count=moduli_count, stream=stream)

    def _respond(self, entry, matrix, rows, cols, queries, galois_keys, baby_step, out_moduli, stream):
        import torch

        word = getattr(torch, self._word.dtype)
        L, n = self.bfv.L, self.bfv.degree
        for name, tensor in (("matrix", matrix), ("queries", queries)):
            if tensor.dtype != word or not tensor.is_cuda or not tensor.is_contiguous():
                raise ValueError(f"{name} must be a contiguous device tensor of the context's words")
        if matrix.dim() != 3 or tuple(matrix.shape[1:]) != (L, n):
            raise ValueError("matrix must be [plaintext_count][L][N]")
        if queries.dim() != 4 or tuple(queries.shape[1:]) != (2, L, n):
            raise ValueError("queries must be [Q][2][L][N]")
        count = queries.shape[0]
        shape = self.matrix_shape(rows, cols, "diagonal", baby_step or 0)
        keys = (vp * (2 * count))()
        if galois_keys is not None:
            if len(galois_keys) != count:
                raise ValueError("galois_keys must hold one (key of -1, key of -baby_step) pair per query")
            for q, pair in enumerate(galois_keys):
                for k, key in enumerate(pair):
                    if key is not None:
                        if key.dtype != word or not key.is_cuda or not key.is_contiguous():
                            raise ValueError("a Galois key must be a contiguous device tensor of the context's words")
                        keys[2 * q + k] = key.data_ptr()
        results = -(-int(rows) // n)
        with torch.cuda.stream(stream) if stream is not None else _no_stream():
            out = _empty((count, results, 2, out_moduli, n), self._word, queries.device)
        _check(_entry(entry, self._word)(self.h, vp(matrix.data_ptr()), matrix.shape[0], int(rows), int(cols),
                                         shape["baby_step"], vp(queries.data_ptr()), count,
                                         keys if galois_keys is not None else None, vp(out.data_ptr()), _stream(stream)))
        return out

    def mul_transpose(self, matrix, rows, cols, queries, galois_keys, baby_step=None, stream=None):
        """he_pnns_mul_transpose_device(_u32): PlaintextMatrix.mulTranspose(vector:using:) for Q one-row queries.  matrix
        [P C][L][N] Eval as diagonal_matrix returns it (baby_step None: the default it was packed with), queries [Q][2][L][N]
        Coeff, galois_keys a list of Q pairs (key of rotatingColumns(by: -1), key of (by: -baby_step)) of device tensors, an
        entry None where the shape does not need it -> [Q][ceil(rows / N)][2][L][N] Coeff."""
        return self._respond("he_pnns_mul_transpose_device", matrix, rows, cols, queries, galois_keys, baby_step, self.bfv.L,
                             stream)

    def compute_response(self, matrix, rows, cols, queries, galois_keys, baby_step=None, stream=None):
        """he_pnns_compute_response_device(_u32): Server.computeResponse for Q one-row queries: mul_transpose, then
        modSwitchDownToSingle -> [Q][ceil(rows / N)][2][1][N] Coeff over q_0."""
        return self._respond("he_pnns_compute_response_device", matrix, rows, cols, queries, galois_keys, baby_step, 1, stream)

    def query_matrix_shape(self, matrix_rows, cols, query_rows):
        """he_pnns_query_matrix_shape -> dict with query_ciphertexts (K), result_ciphertexts (M) and needs: the set of slots of
        galois_keys the shape reads (0..3), plus "pack" for the rotation plan and its keys."""
        k, m, needs = c_size(), c_size(), c_u32()
        _check(load_library().he_pnns_query_matrix_shape(self.h, int(matrix_rows), int(cols), int(query_rows), ctypes.byref(k),
                                                         ctypes.byref(m), ctypes.byref(needs)))
        bits = int(needs.value)
        return {"query_ciphertexts": int(k.value), "result_ciphertexts": int(m.value),
                "needs": {slot for slot in range(4) if bits >> slot & 1} | ({"pack"} if bits >> 4 & 1 else set())}

    def _matrix_entry(self, entry, matrix, rows, cols, queries, query_rows, pack_steps, galois_keys, baby_step, out_moduli,
                      stream):
        import torch

        word = getattr(torch, self._word.dtype)
        L, n = self.bfv.L, self.bfv.degree
        for name, tensor in (("matrix", matrix), ("queries", queries)):
            if tensor.dtype != word or not tensor.is_cuda or not tensor.is_contiguous():
                raise ValueError(f"{name} must be a contiguous device tensor of the context's words")
        if matrix.dim() != 3 or tuple(matrix.shape[1:]) != (L, n):
            raise ValueError("matrix must be [plaintext_count][L][N]")
        if queries.dim() != 5 or tuple(queries.shape[2:]) != (2, L, n):
            raise ValueError("queries must be [Q][K][2][L][N]")
        count = queries.shape[0]
        shape = self.matrix_shape(rows, cols, "diagonal", baby_step or 0)
        query_shape = self.query_matrix_shape(rows, cols, query_rows)
        if queries.shape[1] != query_shape["query_ciphertexts"]:
            raise ValueError("queries must hold ceil(query_rows / rows per ciphertext) ciphertexts per client")
        pack_steps = list(pack_steps or [])
        plan = (PnnsPackStep * max(len(pack_steps), 1))()
        for i, (step, repeat) in enumerate(pack_steps):
            plan[i].step, plan[i].count = int(step), int(repeat)
        stride = 4 + len(pack_steps)
        keys = (vp * (stride * max(count, 1)))()
        if galois_keys is not None:
            if len(galois_keys) != count:
                raise ValueError("galois_keys must hold one list of 4 + len(pack_steps) keys per client")
            for q, row in enumerate(galois_keys):
                if len(row) != stride:
                    raise ValueError("galois_keys must hold one list of 4 + len(pack_steps) keys per client")
                for k, key in enumerate(row):
                    if key is not None:
                        if key.dtype != word or not key.is_cuda or not key.is_contiguous():
                            raise ValueError("a Galois key must be a contiguous device tensor of the context's words")
                        keys[stride * q + k] = key.data_ptr()
        with torch.cuda.stream(stream) if stream is not None else _no_stream():
            out = _empty((count, query_shape["result_ciphertexts"], 2, out_moduli, n), self._word, queries.device)
        _check(_entry(entry, self._word)(self.h, vp(matrix.data_ptr()), matrix.shape[0], int(rows), int(cols),
                                         shape["baby_step"], vp(queries.data_ptr()), int(query_rows), count,
                                         plan if pack_steps else None, len(pack_steps),
                                         keys if galois_keys is not None else None, vp(out.data_ptr()), _stream(stream)))
        return out

    def mul_transpose_matrix(self, matrix, rows, cols, queries, query_rows, pack_steps, galois_keys, baby_step=None,
                             stream=None):
        """he_pnns_mul_transpose_matrix_device(_u32): PlaintextMatrix.mulTranspose(matrix:using:) for Q clients with query
        matrices of query_rows rows.  queries [Q][K][2][L][N] Coeff (dense-row packed), pack_steps the ordered plan of
        rotateColumnsMultiStep(by: rows) as (step, count) pairs, galois_keys per client a list of 4 + len(pack_steps) device
        tensors (keys of -1, -baby_step, swappingRows, P, then the plan's steps), None where the shape does not need one
        -> [Q][M][2][L][N] Coeff, M as query_matrix_shape gives it."""
        return self._matrix_entry("he_pnns_mul_transpose_matrix_device", matrix, rows, cols, queries, query_rows, pack_steps,
                                  galois_keys, baby_step, self.bfv.L, stream)

    def compute_response_matrix(self, matrix, rows, cols, queries, query_rows, pack_steps, galois_keys, baby_step=None,
                                stream=None):
        """he_pnns_compute_response_matrix_device(_u32): Server.computeResponse for such queries: mul_transpose_matrix, then
        modSwitchDownToSingle -> [Q][M][2][1][N] Coeff over q_0."""
        return self._matrix_entry("he_pnns_compute_response_matrix_device", matrix, rows, cols, queries, query_rows,
                                  pack_steps, galois_keys, baby_step, 1, stream)

    # ---- the client's layers: encodeSimd / decodeSimd, the dense packings
    def _plaintext_batch(self, tensor, name):
        import torch

        if (tensor.dtype != getattr(torch, self._word.dtype) or not tensor.is_cuda or not tensor.is_contiguous()
                or tensor.dim() != 2 or tensor.shape[1] != self.bfv.degree):
            raise ValueError(f"{name} must be a contiguous device tensor [batch][N] of the context's words")
        return tensor.shape[0]

    def simd_encode(self, slots, stream=None):
        """he_pnns_simd_encode_device: Context.encodeSimd per row.  slots [batch][N] in slot order (values < t) ->
        (plaintexts [batch][N] Coeff; out_of_range, a one-word int32 device tensor: 1 when a value was not below t)."""
        import torch

        batch, w = self._plaintext_batch(slots, "slots"), self._word
        with torch.cuda.stream(stream) if stream is not None else _no_stream():
            out = _empty((batch, self.bfv.degree), w, slots.device)
            out_of_range = torch.zeros(1, dtype=torch.int32, device=slots.device)
        _check(load_library().he_pnns_simd_encode_device(self.h, w.bits, _ptr(slots, w), batch, _ptr(out, w),
                                                         vp(out_of_range.data_ptr()), _stream(stream)))
        return out, out_of_range

    def simd_decode(self, plaintexts, stream=None):
        """he_pnns_simd_decode_device: Context.decodeSimd per row.  plaintexts [batch][N] Coeff -> slots [batch][N]."""
        import torch

        batch, w = self._plaintext_batch(plaintexts, "plaintexts"), self._word
        with torch.cuda.stream(stream) if stream is not None else _no_stream():
            out = _empty((batch, self.bfv.degree), w, plaintexts.device)
        _check(load_library().he_pnns_simd_decode_device(self.h, w.bits, _ptr(plaintexts, w), batch, _ptr(out, w),
                                                         _stream(stream)))
        return out

    def pack_dense_rows(self, signed_values, reduce=False, stream=None):
        """he_pnns_pack_dense_rows_device: PlaintextMatrix(.denseRow, signedValues:reduce:).  int64 CUDA tensor [rows][cols] ->
        (plaintexts [K][N] Coeff, out_of_range as diagonal_matrix returns it)."""
        import torch

        if (signed_values.dtype != torch.int64 or not signed_values.is_cuda or not signed_values.is_contiguous()
                or signed_values.dim() != 2):
            raise ValueError("signed_values must be a contiguous int64 device tensor [rows][cols]")
        rows, cols = signed_values.shape
        count, w = self.matrix_shape(rows, cols, "denseRow")["plaintext_count"], self._word
        with torch.cuda.stream(stream) if stream is not None else _no_stream():
            out = _empty((count, self.bfv.degree), w, signed_values.device)
            out_of_range = torch.zeros(1, dtype=torch.int32, device=signed_values.device)
        _check(load_library().he_pnns_pack_dense_rows_device(self.h, w.bits, vp(signed_values.data_ptr()), rows, cols,
                                                             int(bool(reduce)), _ptr(out, w), vp(out_of_range.data_ptr()),
                                                             _stream(stream)))
        return out, out_of_range

    def unpack(self, plaintexts, rows, cols, packing="denseColumn", stream=None):
        """he_pnns_unpack_device: PlaintextMatrix.unpack() for "denseColumn" or "denseRow".  plaintexts [count][N] Coeff ->
        int64 tensor [rows][cols] of values below t."""
        import torch

        batch, w = self._plaintext_batch(plaintexts, "plaintexts"), self._word
        number = int(PNNS_PACKINGS.get(packing, packing))
        if number != PNNS_PACKINGS["diagonal"] and batch != self.matrix_shape(rows, cols, number)["plaintext_count"]:
            raise ValueError("plaintexts must hold the packing's plaintext count for rows x cols")
        with torch.cuda.stream(stream) if stream is not None else _no_stream():
            out = torch.empty((int(rows), int(cols)), dtype=torch.int64, device=plaintexts.device)
        _check(load_library().he_pnns_unpack_device(self.h, w.bits, number, _ptr(plaintexts, w), int(rows), int(cols),
                                                    vp(out.data_ptr()), _stream(stream)))
        return out


def _pnns_contexts(contexts):
    contexts = list(contexts)
    if not contexts:
        raise ValueError("one PnnsContext per plaintext modulus")
    handles = (vp * len(contexts))(*[ctx.h for ctx in contexts])
    return contexts, handles, contexts[0]._word


def pnns_generate_query_workspace_bytes(contexts, query_rows, cols):
    contexts, handles, w = _pnns_contexts(contexts)
    return int(load_library().he_pnns_generate_query_workspace_bytes(handles, len(contexts), w.bits, int(query_rows), int(cols)))


def pnns_generate_query(contexts, vectors, scaling_factor, secret_key, a_seeds, error_seeds, stream=None, workspace=None):
    """he_pnns_generate_query_device: Client.generateQuery(for:using:) for a client with one PnnsContext per plaintext modulus.
    vectors float32 CUDA tensor [query_rows][cols], seeds uint8 [contexts][K][32] -> (queries [contexts][K][2][L][N] Coeff,
    out_of_range); queries[c] is one client's `queries` of contexts[c].compute_response_matrix."""
    import torch

    contexts, handles, w = _pnns_contexts(contexts)
    if vectors.dtype != torch.float32 or not vectors.is_cuda or not vectors.is_contiguous() or vectors.dim() != 2:
        raise ValueError("vectors must be a contiguous float32 device tensor [query_rows][cols]")
    rows, cols = vectors.shape
    bfv = contexts[0].bfv
    count = contexts[0].matrix_shape(rows, cols, "denseRow")["plaintext_count"]
    with torch.cuda.stream(stream) if stream is not None else _no_stream():
        out = _empty((len(contexts), count, 2, bfv.L, bfv.degree), w, vectors.device)
        out_of_range = torch.zeros(1, dtype=torch.int32, device=vectors.device)
    ws_ptr, ws_bytes = _workspace(workspace)
    _check(load_library().he_pnns_generate_query_device(
        handles, len(contexts), w.bits, vp(vectors.data_ptr()), rows, cols, float(scaling_factor), _ptr(secret_key, w),
        vp(a_seeds.data_ptr()), vp(error_seeds.data_ptr()), _ptr(out, w), vp(out_of_range.data_ptr()), ws_ptr, ws_bytes,
        _stream(stream)))
    return out, out_of_range


def pnns_decrypt_response_workspace_bytes(contexts, rows, query_rows, moduli_count=1):
    contexts, handles, w = _pnns_contexts(contexts)
    return int(load_library().he_pnns_decrypt_response_workspace_bytes(handles, len(contexts), w.bits, int(moduli_count),
                                                                       int(rows), int(query_rows)))


def pnns_decrypt_response(contexts, response, secret_key, rows, query_rows, scaling_factor, stream=None, workspace=None):
    """he_pnns_decrypt_response_device: Client.decrypt(response:using:).  response [contexts][M][2][moduli_count][N] Coeff (M the
    dense-column plaintext count of rows x query_rows) -> distances, float32 [rows][query_rows]."""
    import torch

    contexts, handles, w = _pnns_contexts(contexts)
    if (response.dtype != getattr(torch, w.dtype) or not response.is_cuda or not response.is_contiguous() or response.dim() != 5
            or response.shape[0] != len(contexts) or response.shape[2] != 2 or response.shape[4] != contexts[0].bfv.degree):
        raise ValueError("response must be a contiguous device tensor [contexts][M][2][moduli_count][N] of the contexts' words")
    if response.shape[1] != contexts[0].matrix_shape(rows, query_rows, "denseColumn")["plaintext_count"]:
        raise ValueError("response must hold the dense-column plaintext count of rows x query_rows per context")
    with torch.cuda.stream(stream) if stream is not None else _no_stream():
        out = torch.empty((int(rows), int(query_rows)), dtype=torch.float32, device=response.device)
    ws_ptr, ws_bytes = _workspace(workspace)
    _check(load_library().he_pnns_decrypt_response_device(
        handles, len(contexts), w.bits, int(response.shape[3]), _ptr(response, w), _ptr(secret_key, w), int(rows),
        int(query_rows), float(scaling_factor), vp(out.data_ptr()), ws_ptr, ws_bytes, _stream(stream)))
    return out


# ---- keyword PIR database: HashKeyword, CuckooTable, HashBucket.serialize ----
class CuckooTableConfig(ctypes.Structure):
    """he_cuckoo_table_config: CuckooTableConfig (KeywordPir/CuckooTable.swift:18-84).  bucket_count given: .fixedSize;
    None: .allowExpansion(expansionFactor:targetLoadFactor:)."""

    _fields_ = [("hash_function_count", c_u32), ("max_eviction_count", c_u32), ("max_serialized_bucket_size", c_u64),
                ("fixed_size", ctypes.c_int), ("bucket_count", c_u64), ("expansion_factor", ctypes.c_double),
                ("target_load_factor", ctypes.c_double), ("multiple_tables", ctypes.c_int), ("slot_count", c_u32)]

    def __init__(self, hash_function_count, max_eviction_count, max_serialized_bucket_size, bucket_count=None,
                 expansion_factor=1.1, target_load_factor=0.9, multiple_tables=True, slot_count=255):
        super().__init__(int(hash_function_count), int(max_eviction_count), int(max_serialized_bucket_size),
                         int(bucket_count is not None), int(bucket_count or 0), float(expansion_factor),
                         float(target_load_factor), int(bool(multiple_tables)), int(slot_count))

    @property
    def table_count(self):
        return self.hash_function_count if self.multiple_tables else 1

    def validate(self):
        _check(load_library().he_keyword_pir_config_validate(ctypes.byref(self)))


def _blob(items, device=None):
    """bytes-like items back to back -> (uint8 array or device tensor, uint64 offsets [len + 1])"""
    offsets = np.zeros(len(items) + 1, dtype=np.uint64)
    np.cumsum([len(item) for item in items], out=offsets[1:])
    blob = np.frombuffer(b"".join(bytes(item) for item in items), dtype=np.uint8).copy()
    if device is None:
        return blob, offsets
    import torch

    return torch.from_numpy(blob).to(device), offsets


def _byte_ptr(tensor):
    if not tensor.is_cuda or tensor.element_size() != 1:
        raise ValueError("expected a uint8 CUDA (HIP) tensor")
    if not tensor.is_contiguous():
        raise ValueError("expected a contiguous tensor")
    return vp(tensor.data_ptr())


def keyword_pir_hash_keywords(keywords, keyword_offsets, stream=None):
    """he_keyword_pir_hash_keywords_device: HashKeyword.hash of keyword i = keywords[offsets[i], offsets[i + 1]) (a uint8
    device tensor, at any byte address; offsets: int64 device tensor [count + 1]) -> int64 tensor [count] of the hashes."""
    import torch

    count = keyword_offsets.numel() - 1
    out = torch.empty((count,), dtype=torch.int64, device=keywords.device)
    _check(load_library().he_keyword_pir_hash_keywords_device(_byte_ptr(keywords), _ptr(keyword_offsets), count, _ptr(out),
                                                              _stream(stream)))
    return out


def keyword_pir_hash_indices(hashes, bucket_count, hash_function_count, stream=None):
    """he_keyword_pir_hash_indices_device: HashKeyword.hashIndices -> int32 tensor [count][hash_function_count]."""
    import torch

    out = torch.empty((hashes.numel(), int(hash_function_count)), dtype=torch.int32, device=hashes.device)
    _check(load_library().he_keyword_pir_hash_indices_device(_ptr(hashes), hashes.numel(), int(bucket_count),
                                                             int(hash_function_count), _ptr(out, WORD32), _stream(stream)))
    return out


def keyword_pir_shard_indices(hashes, shard_count, other_shard_count=0, stream=None):
    """he_keyword_pir_shard_indices_device: ShardingFunction.shardIndex (other_shard_count given: doubleMod) -> int32 [count]."""
    import torch

    out = torch.empty((hashes.numel(),), dtype=torch.int32, device=hashes.device)
    _check(load_library().he_keyword_pir_shard_indices_device(_ptr(hashes), hashes.numel(), int(shard_count),
                                                              int(other_shard_count), _ptr(out, WORD32), _stream(stream)))
    return out


def keyword_pir_bucket_count(config, value_sizes):
    """he_keyword_pir_bucket_count: the bucket count CuckooTable.init starts from.  Host only."""
    sizes = np.ascontiguousarray(value_sizes, dtype=np.uint64)
    out = c_size(0)
    _check(load_library().he_keyword_pir_bucket_count(ctypes.byref(config), sizes.ctypes.data_as(U64P), len(sizes),
                                                      ctypes.byref(out)))
    return out.value


def keyword_pir_cuckoo_place(config, hashes, indices, value_sizes, bucket_count, seed):
    """he_keyword_pir_cuckoo_place on host arrays -> dict(status name, bucket_offsets, slot_entries, placed,
    duplicates_dropped, next_bucket_count); "ok" and "cuckooTableNeedsExpansion" are returned, everything else raises.
    Host only."""
    hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
    sizes = np.ascontiguousarray(value_sizes, dtype=np.uint64)
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    count = len(hashes)
    if len(sizes) != count or indices.size != count * config.hash_function_count:
        raise ValueError("one hash, one size and hash_function_count indices per entry")
    offsets = np.zeros(int(bucket_count) + 1, dtype=np.uint32)
    entries = np.zeros(max(count, 1), dtype=np.uint32)
    placed, dropped, grown = c_size(0), c_size(0), c_size(0)
    u32p = ctypes.POINTER(c_u32)
    status = load_library().he_keyword_pir_cuckoo_place(
        ctypes.byref(config), hashes.ctypes.data_as(U64P), indices.ctypes.data_as(u32p), sizes.ctypes.data_as(U64P), count,
        int(bucket_count), int(seed) & (2**64 - 1), offsets.ctypes.data_as(u32p), entries.ctypes.data_as(u32p),
        ctypes.byref(placed), ctypes.byref(dropped), ctypes.byref(grown))
    if status not in (0, 29):
        _check(status)
    return {"status": STATUS_NAMES[status], "bucket_offsets": offsets, "slot_entries": entries[:placed.value],
            "placed": placed.value, "duplicates_dropped": dropped.value, "next_bucket_count": grown.value}


def keyword_pir_serialize_buckets(hashes, values, value_offsets, bucket_offsets, slot_entries, entry_size_in_bytes, out=None,
                                  mismatch=None, stream=None):
    """he_keyword_pir_serialize_buckets_device: HashBucket.serialize of every bucket of a CSR table (all device tensors: hashes
    and value_offsets int64, bucket_offsets and slot_entries int32, values uint8) -> uint8 [bucket_count][entry_size_in_bytes]
    (out: a contiguous uint8 tensor of that many bytes at any address)."""
    import torch

    buckets = bucket_offsets.numel() - 1
    if out is None:
        out = torch.empty((buckets, int(entry_size_in_bytes)), dtype=torch.uint8, device=hashes.device)
    elif out.numel() != buckets * int(entry_size_in_bytes):
        raise ValueError("out does not hold bucket_count * entry_size_in_bytes bytes")
    _check(load_library().he_keyword_pir_serialize_buckets_device(
        _ptr(hashes), _byte_ptr(values), _ptr(value_offsets), _ptr(bucket_offsets, WORD32), _ptr(slot_entries, WORD32),
        slot_entries.numel(), buckets, int(entry_size_in_bytes), _byte_ptr(out), _opt_ptr(mismatch, WORD32), _stream(stream)))
    return out


class KeywordPirTable:
    """he_keyword_pir_table: CuckooTable.init over a whole database on the device, then serializeBuckets() and the index-PIR
    build per sub-table -- what KeywordPirServer.process does (KeywordPir/KeywordPirProtocol.swift:191-247).

    keywords / values: lists of bytes-like items.  The blobs go to `device` once and `values` stays with the table."""

    def __init__(self, config, keywords, values, seed=0, device="cuda", stream=None):
        if len(keywords) != len(values):
            raise ValueError("one value per keyword")
        self.config = config
        keyword_blob, keyword_offsets = _blob(keywords, device)
        self.values, value_offsets = _blob(values, device)
        handle = vp()
        _check(load_library().he_keyword_pir_table_create_device(
            ctypes.byref(config), vp(keyword_blob.data_ptr()), keyword_offsets.ctypes.data_as(U64P), vp(self.values.data_ptr()),
            value_offsets.ctypes.data_as(U64P), len(keywords), int(seed) & (2**64 - 1), ctypes.byref(handle), _stream(stream)))
        self.h = handle

    def __del__(self):
        if getattr(self, "h", None):
            load_library().he_keyword_pir_table_destroy(self.h)
            self.h = None

    def _get(self, name):
        return getattr(load_library(), "he_keyword_pir_table_" + name)(self.h)

    bucket_count = property(lambda self: self._get("bucket_count"))
    buckets_per_table = property(lambda self: self._get("buckets_per_table"))
    table_count = property(lambda self: self._get("table_count"))
    largest_bucket_size = property(lambda self: self._get("largest_bucket_size"))
    entry_count = property(lambda self: self._get("entry_count"))
    duplicates_dropped = property(lambda self: self._get("duplicates_dropped"))
    expansion_count = property(lambda self: self._get("expansion_count"))
    load_factor = property(lambda self: self._get("load_factor"))

    def entries(self, entry_size_in_bytes=None, out=None, stream=None):
        """he_keyword_pir_table_entries_device -> uint8 [bucket_count][entry_size_in_bytes] (None: the largest bucket)."""
        import torch

        size = self.largest_bucket_size if entry_size_in_bytes is None else int(entry_size_in_bytes)
        if out is None:
            out = torch.empty((self.bucket_count, size), dtype=torch.uint8, device=self.values.device)
        elif out.numel() != self.bucket_count * size:
            raise ValueError("out does not hold bucket_count * entry_size_in_bytes bytes")
        _check(load_library().he_keyword_pir_table_entries_device(self.h, vp(self.values.data_ptr()), size, _byte_ptr(out),
                                                                  _stream(stream)))
        return out

    def process_database(self, context, dimensions, entry_size_in_bytes=None, stream=None):
        """he_keyword_pir_process_database_device with a BfvContext / BfvContext32 -> (database [table_count][chunks][
        prod(dims)][L][N] Eval in the context's words, present uint8 [table_count][chunks][prod(dims)])."""
        import torch

        size = self.largest_bucket_size if entry_size_in_bytes is None else int(entry_size_in_bytes)
        shape = context.pir_database_shape(dimensions, self.buckets_per_table, size, False)
        chunks, per_chunk = shape["chunk_count"], shape["plaintexts_per_chunk"]
        tables = self.table_count
        database = _empty((tables, chunks, per_chunk, context.L, context.degree), context._word, self.values.device)
        present = torch.empty((tables, chunks, per_chunk), dtype=torch.uint8, device=self.values.device)
        dims = (c_u32 * len(dimensions))(*[int(d) for d in dimensions])
        _check(load_library().he_keyword_pir_process_database_device(
            context.h, self.h, vp(self.values.data_ptr()), dims, len(dimensions), size, _ptr(database, context._word),
            vp(present.data_ptr()), _stream(stream)))
        return database, present


# ---- sharded keyword database: Sharding, KeywordDatabase.init ----
class KeywordSharding(ctypes.Structure):
    """he_keyword_sharding: Sharding (KeywordPir/KeywordDatabase.swift:152-242); give shard_count or entry_count_per_shard."""

    _fields_ = [("by_entry_count", ctypes.c_int), ("value", c_u64), ("has_max_shard_count", ctypes.c_int),
                ("max_shard_count", c_u64), ("require_power_of_two", ctypes.c_int)]

    def __init__(self, shard_count=None, entry_count_per_shard=None, max_shard_count=None, require_power_of_two=False):
        if (shard_count is None) == (entry_count_per_shard is None):
            raise ValueError("give shard_count or entry_count_per_shard")
        value = shard_count if entry_count_per_shard is None else entry_count_per_shard
        super().__init__(int(entry_count_per_shard is not None), int(value), int(max_shard_count is not None),
                         int(max_shard_count or 0), int(bool(require_power_of_two)))


def keyword_pir_shard_count(sharding, row_count):
    """he_keyword_sharding_shard_count: Sharding.init's checks and shardCount(for:).  Host only."""
    out = c_size(0)
    _check(load_library().he_keyword_sharding_shard_count(ctypes.byref(sharding), int(row_count), ctypes.byref(out)))
    return out.value


KEYWORD_GATHER_FORMS = {0: "none", 1: "chunk"}


def keyword_pir_partition_plan(count, shard_count, keyword_bytes, value_bytes):
    """he_keyword_database_partition_plan: what keyword_pir_partition runs for a shape.  Host only."""
    passes, tile, key_form, value_form = c_u32(0), c_u32(0), c_u32(0), c_u32(0)
    workgroups, last = c_size(0), c_size(0)
    _check(load_library().he_keyword_database_partition_plan(
        int(count), int(shard_count), int(keyword_bytes), int(value_bytes), ctypes.byref(passes), ctypes.byref(workgroups),
        ctypes.byref(tile), ctypes.byref(last), ctypes.byref(key_form), ctypes.byref(value_form)))
    return {"digit_passes": passes.value, "workgroups_per_pass": workgroups.value, "rows_per_workgroup": tile.value,
            "last_workgroup_rows": last.value, "keyword_gather_form": KEYWORD_GATHER_FORMS[key_form.value],
            "value_gather_form": KEYWORD_GATHER_FORMS[value_form.value]}


def keyword_pir_partition(keywords, keyword_offsets, values, value_offsets, shard_indices, shard_count, mismatch=None,
                          stream=None):
    """he_keyword_database_partition_device: the rows of a database in shard order (device tensors: the blobs uint8, the offsets
    int64 [count + 1], shard_indices int32 [count]) -> dict(keywords, keyword_offsets, values, value_offsets, order int32
    [count], shard_starts int32 [shard_count + 1]).  The blobs' sizes are the tensors'."""
    import torch

    count = shard_indices.numel()
    if keyword_offsets.numel() != count + 1 or value_offsets.numel() != count + 1:
        raise ValueError("count + 1 offsets per blob")
    device = shard_indices.device
    out = {"keywords": torch.empty_like(keywords), "keyword_offsets": torch.empty((count + 1,), dtype=torch.int64, device=device),
           "values": torch.empty_like(values), "value_offsets": torch.empty((count + 1,), dtype=torch.int64, device=device),
           "order": torch.empty((count,), dtype=torch.int32, device=device),
           "shard_starts": torch.empty((int(shard_count) + 1,), dtype=torch.int32, device=device)}
    _check(load_library().he_keyword_database_partition_device(
        _byte_ptr(keywords), _ptr(keyword_offsets), keywords.numel(), _byte_ptr(values), _ptr(value_offsets), values.numel(),
        count, _ptr(shard_indices, WORD32), int(shard_count), _byte_ptr(out["keywords"]), _ptr(out["keyword_offsets"]),
        _byte_ptr(out["values"]), _ptr(out["value_offsets"]), _ptr(out["order"], WORD32), _ptr(out["shard_starts"], WORD32),
        _opt_ptr(mismatch, WORD32), _stream(stream)))
    return out


class _BorrowedBytes:
    """device bytes another object owns, as torch reads them (__cuda_array_interface__)"""

    def __init__(self, address, nbytes, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (address, False), "version": 2}


class KeywordPirShardTable(KeywordPirTable):
    """The table of one shard of a KeywordPirShardedDatabase: every query and method of KeywordPirTable over a handle the
    database owns."""

    def __init__(self, handle, values, config, database):
        self.h, self.values, self.config, self.database = handle, values, config, database

    def __del__(self):
        self.h = None  # the database destroys its tables


class KeywordPirShardedDatabase:
    """he_keyword_database: KeywordDatabase.init(rows:sharding:shardingFunction:) on the device
    (KeywordPir/KeywordDatabase.swift:406-437) -- hash, shard, partition, one cuckoo table per shard that received a row.

    keywords / values: lists of bytes-like items; shard_count: a count or a KeywordSharding; other_shard_count: doubleMod.
    shards() yields (KeywordPirShardTable or None, the shard's values as a uint8 tensor into the object's blob)."""

    def __init__(self, config, keywords, values, shard_count, other_shard_count=0, seed=0, device="cuda", stream=None):
        if len(keywords) != len(values):
            raise ValueError("one value per keyword")
        if isinstance(shard_count, KeywordSharding):
            shard_count = keyword_pir_shard_count(shard_count, len(keywords))
        self.config, self.device = config, device
        keyword_blob, keyword_offsets = _blob(keywords, device)
        value_blob, value_offsets = _blob(values, device)
        handle = vp()
        _check(load_library().he_keyword_database_create_device(
            ctypes.byref(config), vp(keyword_blob.data_ptr()), keyword_offsets.ctypes.data_as(U64P), vp(value_blob.data_ptr()),
            value_offsets.ctypes.data_as(U64P), len(keywords), int(shard_count), int(other_shard_count),
            int(seed) & (2**64 - 1), ctypes.byref(handle), _stream(stream)))
        self.h = handle
        self._value_sizes = np.diff(value_offsets.astype(np.int64))
        self._bounds = None

    def __del__(self):
        if getattr(self, "h", None):
            load_library().he_keyword_database_destroy(self.h)
            self.h = None

    @property
    def shard_count(self):
        return load_library().he_keyword_database_shard_count(self.h)

    def shard_row_count(self, shard):
        return load_library().he_keyword_database_shard_row_count(self.h, int(shard))

    def order(self):
        """he_keyword_database_order -> uint32 array [count]: shard after shard, the input rows each holds"""
        out = np.zeros(len(self._value_sizes), dtype=np.uint32)
        _check(load_library().he_keyword_database_order(self.h, out.ctypes.data_as(ctypes.POINTER(c_u32))))
        return out

    def _shard_bytes(self):
        """(first row, first value byte) of every shard and of the end, from the order and the row counts, once"""
        if self._bounds is None:
            rows = np.array([self.shard_row_count(s) for s in range(self.shard_count)], dtype=np.int64)
            starts = np.concatenate(([0], np.cumsum(rows)))
            running = np.concatenate(([0], np.cumsum(self._value_sizes[self.order()])))
            self._bounds = starts, running[starts]
        return self._bounds

    def shard(self, shard):
        """(KeywordPirShardTable, values tensor) of one shard, or (None, an empty tensor) where it received no row"""
        import torch

        lib = load_library()
        shard = int(shard)
        table = lib.he_keyword_database_shard_table(self.h, shard)
        if not table:
            return None, torch.empty((0,), dtype=torch.uint8, device=self.device)
        _, byte_starts = self._shard_bytes()
        nbytes = int(byte_starts[shard + 1] - byte_starts[shard])
        if nbytes == 0:
            values = torch.empty((0,), dtype=torch.uint8, device=self.device)
        else:
            address = lib.he_keyword_database_shard_values(self.h, shard)
            values = torch.as_tensor(_BorrowedBytes(address, nbytes, self), device=self.device)
        return KeywordPirShardTable(vp(table), values, self.config, self), values

    def shards(self):
        for shard in range(self.shard_count):
            yield self.shard(shard)


def _no_stream():
    import contextlib

    return contextlib.nullcontext()
