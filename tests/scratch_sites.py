"""Every place in csrc/ that takes library-owned scratch, and the case of tests/test_gpu_scratch_poison.py that goes through it.

A site is one declaration of `Scratch` or `ZeroizedWorkspace` objects (or a direct scratch_allocate call): (file, enclosing
function, the declared names).  tests/test_scratch_sites.py greps csrc/ and holds this table to exactly the sites it finds.

Per site: the C entry of include/he_amd.h that reaches it and the named case that makes that call --
  * a row of tests/footprint_cases.py WORKSPACE (the row's name): test_workspace_pipelines_on_library_scratch runs it with
    `workspace = NULL` at every shape;
  * a key of DELEGATED: a test of the entry's own file, at its smallest shape, run under the switch by
    test_entries_that_own_their_scratch.  Those tests compare with their reference themselves.
`reached` is None, or why no case reaches the site: the source condition that keeps a few-second shape away from it
(in backquotes), or a second device (device_group.cpp).  tests/test_scratch_sites.py allows at most four of the first kind.

What is checked and what is read: the poison test checks that a DELEGATED case calls every entry the table names for it and,
with the cache keeping everything, that library scratch was taken.  That the call then passes through the very declaration of
the row -- the ones of pnns_api.cpp mul_transpose_matrix and bsgs_product stand behind shape-dependent branches -- was read in
the source at the case's shape, not observed."""
import collections
import importlib

Site = collections.namedtuple("Site", "file function names entry case reached")
SECOND_DEVICE = "needs a second device"
CALLERS_WORKSPACE = ("simple_pir_client_api.cpp resolve_workspace: `if (workspace == nullptr) return invalid_argument(...)` -- these "
                     "entries take no scratch of the library's")


def site(file, function, names, entry, case, reached=None):
    return Site(file, function, names, entry, case, reached)


SITES = [
    # ---- the scheme level (bfv_api.cpp)
    site("bfv_api.cpp", "mul_pipeline", "scratch", "he_bfv_mul_device", "he_bfv_mul_device"),
    site("bfv_api.cpp", "relinearize_pipeline", "scratch", "he_bfv_relinearize_device", "he_bfv_relinearize_device"),
    site("bfv_api.cpp", "bfv_apply_galois_grouped", "scratch", "he_bfv_apply_galois_device", "he_bfv_apply_galois_device"),
    site("bfv_api.cpp", "decrypt_words", "scratch", "he_bfv_decrypt_device", "he_bfv_decrypt_device"),
    site("bfv_api.cpp", "noise_norm_words", "scratch", "he_bfv_noise_norm_device", "he_bfv_noise_norm_device"),
    site("bfv_api.cpp", "he_bfv_secret_dot_product_device", "scratch", "he_bfv_secret_dot_product_device",
         "he_bfv_secret_dot_product_device"),
    site("bfv_api.cpp", "bfv_mod_switch_down_to_single", "level_mem", "he_bfv_mod_switch_down_to_single_device", "mod-switch-to-single"),
    site("bfv_api.cpp", "he_bfv_inner_product_plain_device", "scratch", "he_bfv_inner_product_plain_device", "inner-product-plain"),
    site("bfv_api.cpp", "inner_product_pipeline", "scratch", "he_bfv_inner_product_device", "he_bfv_inner_product_device"),
    site("bfv_api.cpp", "inner_product_shared_pipeline", "scratch", "he_bfv_inner_product_shared_device", "inner-product-shared"),
    site("bfv_api.cpp", "bfv_inner_product_shared_eval_rhs", "scratch coeff_mem", "he_pir_compute_response_chunk_device",
         "pir-eval-rows"),
    # ---- polynomials and the wire format (c_api.cpp)
    site("c_api.cpp", "poly_mul_scalar", "scratch", "he_poly_mul_scalar_device", "poly-known-answers"),
    site("c_api.cpp", "poly_random_from_seeds", "chain", "he_poly_random_from_seeds_device", "seeded-polynomials"),
    site("c_api.cpp", "ciphertexts_deserialize_seeded", "chain", "he_ciphertexts_deserialize_seeded_device", "seeded-ciphertexts"),
    # ---- the device group (device_group.cpp)
    site("device_group.cpp", "dim0_columns_group", "query_copy shard_out", "he_pir_dim0_columns_group", None, SECOND_DEVICE),
    site("device_group.cpp", "response_by_whole_chunks", "dim0_copy remaining_copy key_copy shard_out", "he_pir_compute_response_group",
         None, SECOND_DEVICE),
    site("device_group.cpp", "he_pir_compute_response_group", "intermediate", "he_pir_compute_response_group", None, SECOND_DEVICE),
    # ---- keys and encryption (encrypt_api.cpp)
    site("encrypt_api.cpp", "encrypt_zero_entry", "ws", "he_bfv_encrypt_zero_device", "he_bfv_encrypt_zero_device"),
    site("encrypt_api.cpp", "key_switch_keys_entry", "ws", "he_bfv_generate_key_switch_keys_device",
         "he_bfv_generate_key_switch_keys_device"),
    site("encrypt_api.cpp", "poly_sample", "ws", "he_poly_random_ternary_from_seeds_device", "samplers"),
    site("encrypt_api.cpp", "he_bfv_generate_secret_key_device", "ws", "he_bfv_generate_secret_key_device",
         "he_bfv_generate_secret_key_device"),
    # ---- keyword PIR
    site("keyword_pir_api.cpp", "serialize_buckets", "starts", "he_keyword_pir_serialize_buckets_device", "keyword-serialize"),
    site("keyword_pir_api.cpp", "process_database", "entries_mem", "he_keyword_pir_process_database_device", "keyword-end-to-end"),
    site("keyword_pir_api.cpp", "he_keyword_pir_table_create_device", "hashes_mem offsets_mem", "he_keyword_pir_table_create_device",
         "keyword-end-to-end"),
    site("keyword_pir_api.cpp", "keyword_pir_table_from_hashes", "indices_mem", "he_keyword_pir_table_create_device",
         "keyword-end-to-end"),
    site("keyword_pir_client_api.cpp", "he_keyword_client_generate_query_device", "ws", "he_keyword_client_generate_query_device",
         "keyword-end-to-end"),
    site("keyword_pir_client_api.cpp", "he_keyword_client_find_in_buckets_device", "ws", "he_keyword_client_find_in_buckets_device",
         "keyword-find"),
    site("keyword_pir_client_api.cpp", "he_keyword_client_decrypt_response_device", "ws", "he_keyword_client_decrypt_response_device",
         "keyword-end-to-end"),
    site("keyword_pir_client_api.cpp", "he_keyword_client_count_entries_device", "ws", "he_keyword_client_count_entries_device",
         "keyword-end-to-end"),
    site("keyword_shard_api.cpp", "he_keyword_database_partition_device", "alternate counts sums tile_rows",
         "he_keyword_database_partition_device", "keyword-partition"),
    site("keyword_shard_api.cpp", "he_keyword_database_create_device",
         "offsets_mem out_offsets_mem hashes_mem sorted_mem indices_mem order_mem starts_mem", "he_keyword_database_create_device",
         "keyword-shards"),
    # ---- index PIR
    site("pir_api.cpp", "remaining_dimensions", "next_mem products_mem", "he_pir_compute_response_device", "pir-response"),
    site("pir_api.cpp", "response_chunks_resident", "results_mem", "he_pir_compute_response_device", "pir-response"),
    site("pir_api.cpp", "compute_response_queries", "all_mem one_mem", "he_pir_compute_response_to_query_device", "pir-end-to-end"),
    site("pir_api.cpp", "he_pir_compute_response_chunk_device", "mask_mem", "he_pir_compute_response_chunk_device", "pir-chunk"),
    site("pir_api.cpp", "he_pir_expand_batch_device", "cur_mem next_mem parent_mem rotated_mem tmp_mem workspace_mem",
         "he_pir_expand_device", "pir-expand"),
    site("pir_api.cpp", "compute_response_to_query", "expanded_mem query_mem wide_mem side_mem",
         "he_pir_compute_response_to_query_device", "pir-end-to-end"),
    site("pir_client_api.cpp", "generate_query", "ws", "he_pir_generate_query_device", "pir-end-to-end"),
    site("pir_client_api.cpp", "decrypt_response", "ws", "he_pir_decrypt_response_device", "pir-end-to-end"),
    site("pir_database.cpp", "process_database", "sizes_mem", "he_pir_process_database_device", "pir-end-to-end"),
    site("pir_database.cpp", "process_database", "staging_mem", "he_pir_process_database_device", "pir-end-to-end"),
    site("pir_database_file.cpp", "database_load", "ranks", "he_pir_database_load_device", "pir-database-file"),
    site("pir_database_file.cpp", "database_save", "ranks", "he_pir_database_save_device", "pir-database-file"),
    # ---- PNNS
    site("pnns_api.cpp", "diagonal_matrix", "staging_mem", "he_pnns_diagonal_matrix_device", "pnns-response"),
    site("pnns_api.cpp", "bsgs_product", "rot_mem", "he_pnns_compute_response_device", "pnns-response"),
    site("pnns_api.cpp", "bsgs_product", "products_mem sums_mem", "he_pnns_compute_response_device", "pnns-response"),
    site("pnns_api.cpp", "mul_transpose_matrix", "rows_mem", "he_pnns_compute_response_matrix_device", "pnns-response-matrix"),
    site("pnns_api.cpp", "mul_transpose_matrix", "staging_mem masks_mem eval_mem copies_mem", "he_pnns_compute_response_matrix_device",
         "pnns-response-matrix"),
    site("pnns_api.cpp", "mul_transpose_matrix", "results_mem single_mem", "he_pnns_compute_response_matrix_device",
         "pnns-response-matrix"),
    site("pnns_api.cpp", "mul_transpose_matrix", "sums_mem", "he_pnns_compute_response_matrix_device", "pnns-response-matrix"),
    site("pnns_client_api.cpp", "simd_decode", "ws", "he_pnns_simd_decode_device", "pnns-simd"),
    site("pnns_client_api.cpp", "unpack", "ws", "he_pnns_unpack_device", "pnns-unpack"),
    site("pnns_client_api.cpp", "generate_query", "ws", "he_pnns_generate_query_device", "pnns-client"),
    site("pnns_client_api.cpp", "decrypt_response", "ws", "he_pnns_decrypt_response_device", "pnns-client"),
    # ---- SimplePIR
    site("simple_pir_api.cpp", "process_database", "table_mem chain_mem a_mem a_eval_mem", "he_simple_pir_process_database_device",
         "simple-pir-server"),
    site("simple_pir_api.cpp", "process_database", "staging_mem rows_mem", "he_simple_pir_process_database_device",
         "simple-pir-server"),
    # (the SimplePIR client's workspaces are always the caller's: its ZeroizedWorkspace only zeroizes them)
    site("simple_pir_client_api.cpp", "he_simple_pir_encrypt_zero_device", "ws", "he_simple_pir_encrypt_zero_device", None,
         CALLERS_WORKSPACE),
    site("simple_pir_client_api.cpp", "he_simple_pir_secret_times_hint_device", "ws", "he_simple_pir_secret_times_hint_device", None,
         CALLERS_WORKSPACE),
    site("simple_pir_client_api.cpp", "he_simple_pir_precompute_queries_device", "ws", "he_simple_pir_precompute_queries_device", None,
         CALLERS_WORKSPACE),
    site("simple_pir_client_api.cpp", "he_simple_pir_decrypt_responses_device", "ws", "he_simple_pir_decrypt_responses_device", None,
         CALLERS_WORKSPACE),
    site("simple_pir_shard_api.cpp", "he_simple_pir_shard_map_device", "sums scan", "he_simple_pir_shard_map_device",
         "simple-pir-shards"),
]

# name: (module of tests/, test function, its arguments).  An argument that is a string starting with "=" is an expression over the
# module's own names and `oracle` (what the module's fixture of that name would build); the fixtures oracle, kats, monkeypatch and
# tmp_path are handed in by name.
DELEGATED = {
    # (nine ciphertext moduli: the one-kernel form ends at eight, `sizeof(W) == 8`: "one kernel for 2..8 moduli")
    "mod-switch-to-single": ("test_gpu_bfv", "test_mod_switch_down_to_single", {"bits": [60, 61, 62, 55, 50, 45, 40, 58, 59, 57]}),
    "inner-product-plain": ("test_gpu_bfv", "test_inner_product_plain_reduction_cadence", {"bits": [62, 62, 62]}),
    "inner-product-shared": ("test_gpu_bfv", "test_inner_product_shared_left_vector", {"bits": [50, 50, 50], "count": 4, "items": 1}),
    "poly-known-answers": ("test_gpu_poly", "test_poly_ops_known_answers", {}),
    "seeded-polynomials": ("test_gpu_wire_format_edges", "test_seeded_polynomials_at_counter_carries",
                           {"degree": 64, "bits": [30, 31, 33]}),
    "seeded-ciphertexts": ("test_gpu_ciphertext_wire", "test_deserialize_seeded", {"degree": 8, "rows": 3, "word_bits": 64}),
    "samplers": ("test_gpu_encrypt", "test_samplers_word_for_word", {"degree": 8, "bits": [30], "word": 64, "batch": 1}),
    "keyword-end-to-end": ("test_gpu_keyword_pir_client", "test_keywords_to_values_on_the_device", {"degree": 64, "mode": "pack"}),
    "keyword-find": ("test_gpu_keyword_pir_client", "test_find_in_a_batch_of_distinct_rows", {"form": "staged"}),
    "keyword-serialize": ("test_gpu_keyword_pir", "test_serialized_buckets", {"name": "empty buckets of one byte", "offset": 0}),
    "keyword-partition": ("test_gpu_keyword_shard", "test_partition_through_the_binding", {}),
    "keyword-shards": ("test_gpu_keyword_shard", "test_sharded_database_end_to_end",
                       {"context": "=heamd.BfvContext(DEGREE, heamd.generate_primes([17], True, DEGREE)[0], "
                                   "heamd.generate_primes([40, 40, 40, 41], False, DEGREE))",
                        "database": "=(lambda kv: (kv[0] + kv[0][10:16], kv[1] + [b'later' + bytes([k]) for k in range(6)]))"
                                    "(cases.database(200, count=194))",
                        "config_name": "two tables, expansion allowed", "other_shard_count": 8}),
    "pir-response": ("test_gpu_footprint", "test_pir_compute_response_footprint", {"bits": 64}),
    "pir-chunk": ("test_gpu_decrypt", "test_a_pir_response_decrypts_on_the_device", {}),
    # (`qbsk.log_degree < 12` returns before bfv_inner_product_shared_eval_rhs's site: N = 4096, a 16 x 8 chunk)
    "pir-eval-rows": ("test_gpu_pir", "test_pir_response_config_shape", {"degree": 4096, "bits": [55, 55, 55]}),
    "pir-expand": ("test_gpu_footprint", "test_pir_expand_footprint", {"total": 8}),
    "pir-end-to-end": ("test_gpu_pir_client", "test_indices_to_entries_on_the_device", {"degree": 64, "mode": "pack"}),
    "pir-database-file": ("test_gpu_pir_database_file", "test_processed_database_round_trips_through_its_file", {"word32": False}),
    "pnns-response": ("test_gpu_footprint", "test_pnns_compute_response_footprint", {"word32": False}),
    "pnns-response-matrix": ("test_gpu_footprint", "test_pnns_compute_response_matrix_footprint", {"word32": False}),
    "pnns-simd": ("test_gpu_pnns_client", "test_simd_encode_and_decode", {"degree": 64, "word32": False}),
    "pnns-unpack": ("test_gpu_pnns_client", "test_unpack_dense_columns", {"degree": 64, "rows": 10, "cols": 5, "word32": False}),
    "pnns-client": ("test_gpu_pnns_client", "test_float_queries_to_float_distances",
                    {"degree": 64, "contexts": 1, "rows": 10, "cols": 4, "query_rows": 5}),
    # (a Case of its own: the module's fixture keeps the ones it built, and a kept one makes no call)
    "simple-pir-server": ("test_gpu_simple_pir", "test_database_and_hint", {"case": "=Case('one-entry-u64')"}),

    "simple-pir-shards": ("test_gpu_simple_pir_shards", "test_end_to_end_on_the_device",
                          {"plaintext_bits": 14, "ciphertext_bits": 42, "word_bits": 64}),
}
FIXTURES = ("oracle", "kats", "monkeypatch", "tmp_path")


def resolve(case, request):
    """-> (the test function, its arguments) of a DELEGATED case, inside a running test"""
    import inspect

    module_name, function_name, given = case
    module = importlib.import_module(module_name)
    function = getattr(module, function_name)
    arguments = {}
    for name in inspect.signature(function).parameters:
        if name in given:
            value = given[name]
            if isinstance(value, str) and value.startswith("="):
                value = eval(value[1:], dict(vars(module), oracle=request.getfixturevalue("oracle")))  # noqa: S307
            arguments[name] = value
        else:
            assert name in FIXTURES, (module_name, function_name, name)
            arguments[name] = request.getfixturevalue(name)
    return function, arguments
