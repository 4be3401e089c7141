"""What tests/aliasing_cases.py lacks for running its rows on real memory (tests/test_gpu_footprint.py): per row what every slab
holds when the call starts, which `*_workspace_bytes` function sizes its workspace, and the shapes it runs at.

Fill kinds (FILLS[row][slab]); every input is valid for its entry -- this table is about memory, not about garbage operands:
  q         residues [..][rows of the call's moduli][N], row r below q_r (a polynomial context: all its moduli; a scheme
            context: the first L ciphertext moduli); the first item's rows hold 0, the last item's q_r - 1
  all       the same over EVERY coefficient moduli of a scheme context: secret keys over the secret-key context, key-switching
            keys [TOP][2][TOP + 1][N] over the key-switching context
  qbsk      the same over the 2 L + 1 moduli of the extended base [Q, Bsk] (a lifted slab)
  t         values [..][N] below the plaintext modulus (first item 0, last item t - 1)
  seeds     32-byte seeds: uniform bytes
  bytes     uniform bytes: serialized records (their fields are not validated, he_amd.h), narrow words
  words32   8-byte words below 2^30 (what he_words_narrow_u64_device takes)
  flags     bytes that are 0 or 1
  acc       (low, high) pairs of a lazy accumulator: any low word, a high word below 2^20
  zero      a word the caller zeroes and the entry may set (device_header_mismatch)
  packed    packed plaintexts: zero bits (the polynomial 0; the layout is the packing kernel's own)
  out       a pure output: poisoned
  workspace the caller's workspace: poisoned
A slab the row writes whose kind is none of the last two is updated in place: it holds its input and is not poisoned.

WORKSPACE[row] = (size function of include/he_amd.h, its arguments behind the context as expressions over the row's
environment).  The `_u32` twins take HALF the bytes the function reports (he_amd.h, "Workspaces: half the bytes ..."); the entries
that take word_bits hand it to the function.

Shapes.  Every row and word runs at SMALL (the table's ring, N = 8; N = 256 for the packed-plaintext rows) and at TILED
(N = 4096, batch 3, four moduli of 55 bits on 8-byte words and of 27, 28, 28, 29 bits on 4-byte words: several workgroups, row
pairs and an odd row).  The workspace pipelines run at one more shape per kernel form their launchers can take (FORMS), each
with the source condition that selects the form.  The library gives no way to observe the form a call took: every shape follows
from the condition as read in csrc/bfv_api.cpp, csrc/ntt_routing.hip and csrc/behz_kernels.hip (kOneGeneration = 512 rows,
csrc/ntt_rows.hpp; kBehzRowsFusedAbove = 1152).
"""
import collections

import aliasing_cases as A

RECORD = A.RECORD
FILLS = {
    "he_poly_add_device": {"lhs": "q", "rhs": "q"},
    "he_poly_sub_device": {"lhs": "q", "rhs": "q"},
    "he_poly_mul_device": {"lhs": "q", "rhs": "q"},
    "he_poly_divide_and_round_q_last_device": {"in": "q", "out": "out"},
    "he_poly_adding_lazy_product_device": {"lhs": "q", "rhs": "q", "acc_lo_hi": "acc"},
    "he_poly_reduce_accumulator_device": {"acc_lo_hi": "acc", "out": "out"},
    "he_poly_apply_galois_device": {"in": "q", "out": "out"},
    "he_poly_multiply_power_of_x_device": {"in": "q", "out": "out"},
    "he_poly_serialize_device": {"device_slab": "q", "device_bytes": "out"},
    "he_poly_deserialize_device": {"device_bytes": "bytes", "device_slab": "out"},
    "he_poly_random_from_seeds_device": {"device_seeds": "seeds", "device_slab": "out"},
    "he_ciphertexts_serialize_device": {"cts": "q", "records": "out"},
    "he_ciphertexts_deserialize_device": {"records": "bytes", "cts": "out", "device_header_mismatch": "zero"},
    "he_ciphertexts_deserialize_seeded_device": {"poly0_bytes": "bytes", "seeds": "seeds", "cts": "out"},
    "he_words_widen_u32_device": {"device_in": "bytes", "device_out": "out"},
    "he_words_narrow_u64_device": {"device_in": "words32", "device_out": "out"},
    "he_words_copy_device": {"device_in": "bytes", "device_out": "out"},
    "he_rns_lift_q_to_qbsk_device": {"in": "q", "out": "out"},
    "he_rns_floor_qbsk_to_q_device": {"in": "qbsk", "out": "out"},
    "he_rns_scale_and_round_device": {"in": "q", "out": "out"},
    "he_bfv_mul_device": {"lhs": "q", "rhs": "q", "out": "out", "workspace": "workspace"},
    "he_bfv_relinearize_device": {"ct3": "q", "key": "all", "out": "out", "workspace": "workspace"},
    "he_bfv_apply_galois_device": {"ct": "q", "galois_key": "all", "out": "out", "workspace": "workspace"},
    "he_bfv_apply_galois_grouped_device": {"ct": "q", "galois_keys[0]": "all", "galois_keys[1]": "all", "out": "out",
                                           "workspace": "workspace"},
    "he_bfv_mod_switch_down_device": {"in": "q", "out": "out"},
    "he_bfv_mod_switch_down_to_single_device": {"in": "q", "out": "out"},
    "he_bfv_mul_plain_device": {"ct": "q", "pt": "q"},
    "he_bfv_add_plain_device": {"ct": "q", "plaintexts": "t"},
    "he_bfv_sub_plain_device": {"ct": "q", "plaintexts": "t"},
    "he_bfv_inner_product_plain_device": {"cts": "q", "pts": "q", "out": "out"},
    "he_bfv_inner_product_plain_resident_device": {"cts": "q", "pts": "q", "present_device": "flags", "out": "out"},
    "he_bfv_pack_plaintexts_device": {"plaintexts_eval": "q", "packed": "out"},
    "he_bfv_inner_product_plain_packed_device": {"cts": "q", "packed_pts": "packed", "present_device": "flags", "out": "out"},
    "he_bfv_inner_product_device": {"lhs": "q", "rhs": "q", "out": "out", "workspace": "workspace"},
    "he_bfv_inner_product_shared_device": {"lhs": "q", "rhs": "q", "out": "out"},
    "he_bfv_plaintext_to_eval_device": {"plaintext": "t", "out": "out"},
    "he_bfv_plaintext_to_coeff_device": {"plaintext_eval": "q", "out": "out"},
    "he_bfv_secret_dot_product_device": {"cts": "q", "secret_key": "q", "out": "out", "workspace": "workspace"},
    "he_bfv_decrypt_device": {"cts": "q", "secret_key": "q", "out_plaintexts": "out", "workspace": "workspace"},
    "he_bfv_noise_norm_device": {"cts": "q", "secret_key": "q", "out_limbs": "out", "workspace": "workspace"},
    "he_bfv_is_transparent_device": {"cts": "q", "out_flags": "out"},
    "he_bfv_generate_secret_key_device": {"seeds": "seeds", "out": "out", "workspace": "workspace"},
    "he_bfv_encrypt_zero_device": {"secret_key": "q", "a_seeds": "seeds", "error_seeds": "seeds", "out": "out",
                                   "workspace": "workspace"},
    "he_bfv_encrypt_device": {"secret_key": "q", "a_seeds": "seeds", "error_seeds": "seeds", "plaintexts": "t", "out": "out",
                              "workspace": "workspace"},
    "he_bfv_generate_key_switch_keys_device": {"secret_key": "all", "current_keys": "all", "a_seeds": "seeds",
                                               "error_seeds": "seeds", "out": "out", "workspace": "workspace"},
    "he_bfv_generate_relinearization_key_device": {"secret_key": "all", "a_seeds": "seeds", "error_seeds": "seeds", "out": "out",
                                                   "workspace": "workspace"},
    "he_bfv_generate_galois_keys_device": {"secret_key": "all", "a_seeds": "seeds", "error_seeds": "seeds", "out": "out",
                                           "workspace": "workspace"},
    "he_poly_random_ternary_from_seeds_device": {"seeds": "seeds", "out": "out"},
    "he_poly_random_centered_binomial_from_seeds_device": {"seeds": "seeds", "out": "out"},
}
POISONED = ("out", "workspace")

# he_encrypt_operation of include/he_amd.h
OP_SECRET_KEY, OP_ENCRYPT_ZERO, OP_ENCRYPT, OP_KEY_SWITCH_KEYS, OP_RELINEARIZATION_KEY, OP_GALOIS_KEYS = range(6)
WORKSPACE = {
    "he_bfv_mul_device": ("he_bfv_mul_workspace_bytes", "L batch"),
    "he_bfv_relinearize_device": ("he_bfv_relinearize_workspace_bytes", "L batch"),
    "he_bfv_apply_galois_device": ("he_bfv_apply_galois_workspace_bytes", "L batch"),
    "he_bfv_apply_galois_grouped_device": ("he_bfv_apply_galois_workspace_bytes", "L 2*batch"),  # groups * group_size
    "he_bfv_inner_product_device": ("he_bfv_inner_product_workspace_bytes", "L count"),
    "he_bfv_secret_dot_product_device": ("he_bfv_decrypt_workspace_bytes", "word_bits L polys is_eval batch"),
    "he_bfv_decrypt_device": ("he_bfv_decrypt_workspace_bytes", "word_bits L polys is_eval batch"),
    "he_bfv_noise_norm_device": ("he_bfv_decrypt_workspace_bytes", "word_bits L polys is_eval batch"),
    "he_bfv_generate_secret_key_device": ("he_bfv_encrypt_workspace_bytes", "word_bits %d L 0 batch" % OP_SECRET_KEY),
    "he_bfv_encrypt_zero_device": ("he_bfv_encrypt_workspace_bytes", "word_bits %d L eval_out batch" % OP_ENCRYPT_ZERO),
    "he_bfv_encrypt_device": ("he_bfv_encrypt_workspace_bytes", "word_bits %d L 0 batch" % OP_ENCRYPT),
    "he_bfv_generate_key_switch_keys_device": ("he_bfv_encrypt_workspace_bytes", "word_bits %d TOP 0 keys" % OP_KEY_SWITCH_KEYS),
    "he_bfv_generate_relinearization_key_device": ("he_bfv_encrypt_workspace_bytes",
                                                   "word_bits %d TOP 0 1" % OP_RELINEARIZATION_KEY),
    "he_bfv_generate_galois_keys_device": ("he_bfv_encrypt_workspace_bytes", "word_bits %d TOP 0 count" % OP_GALOIS_KEYS),
}
# The six workspace pipelines whose words are held to the oracle at every shape, and the decrypt dot product
ORACLE_ROWS = ("he_bfv_mul_device", "he_bfv_relinearize_device", "he_bfv_apply_galois_device",
               "he_bfv_apply_galois_grouped_device", "he_bfv_inner_product_device", "he_bfv_secret_dot_product_device")

# Parameters that follow from the ring (the table's literals are for N = 8 on fake addresses): records lie back to back -- a
# serializer leaves the bytes between a record's end and its stride alone (he_amd.h), which would keep the poison inside a
# written slab; those gaps are the wire-format tests' (tests/test_gpu_ciphertext_wire.py guards them).
DERIVED = {
    "he_poly_deserialize_device": {"bytes_per_poly": RECORD},
    "he_ciphertexts_serialize_device": {"stride": "2+polys*(%s)" % RECORD},
    "he_ciphertexts_deserialize_device": {"stride": "2+polys*(%s)" % RECORD},
    "he_ciphertexts_deserialize_seeded_device": {"stride": RECORD},
}

Shape = collections.namedtuple("Shape", "name degree bits overrides setenv alias why")
BITS_SMALL = {64: A.RINGS["small"][1], 32: A.RINGS["small"][1]}
BITS_TILED = {64: (55, 55, 55, 55), 32: (27, 28, 28, 29)}
BITS_TILED_64 = {64: (55, 55, 55, 55)}


def shape(name, degree, bits, why, setenv=None, alias=None, **overrides):
    """degree None: the row's ring of tests/aliasing_cases.py.  bits: {slab word: bits of the coefficient moduli} -- a word
    that is not a key does not run.  alias (written, read): the written slab is passed at the read one's address, a form the
    row's `same` allows: the call updates the head of the read slab in place."""
    return Shape(name, degree, bits, overrides, setenv or {}, alias, why)


SMALL = shape("N8", None, BITS_SMALL, "the table's ring: fewer coefficients than a wavefront, no tiled transform")
TILED = shape("N4096", 4096, BITS_TILED, "test_gpu_aliasing.SHAPES: several workgroups, row pairs, an odd row",
              batch=3, L=3, words=3 * 4096 + 7)
BELOW = "a level below the top: L = 2 of TOP = 3, the key's rows TOP + 1 apart"

FORMS = {
    # ---- ct x ct (bfv_api.cpp mul_pipeline); rows = 2 L + 1
    "he_bfv_mul_device": [
        # SMALL: ntt_routing.hip launch_ntt_tensor_inverse `!tiled` (log_degree < 12): the unfused form -- the lift writes the
        #   copy, ntt_records, launch_tensor, drop_extended_base
        # TILED: launch_ntt_tensor_inverse `12 <= log_degree <= kMaxFusedLoadLogDegree`, records * rows = 63 <= kOneGeneration: one
        #   launch forms the products as the inverse transform loads; ntt_lifted_forward_supported false (items * 4 * rows = 84
        #   <= kOneGeneration): the lift writes the copy
        shape("N4096-lift-from-source", 4096, BITS_TILED,
              "ntt_lifted_forward_supported: records * record_rows = 25 * 4 * 7 = 700 > kOneGeneration (and headroom_prefix == L): "
              "the lift does not write the copy; launch_ntt_tensor_inverse: 25 * 3 * 7 = 525 > kOneGeneration: one launch per "
              "band run; behz_rows_fused_supported false: 25 * 7 = 175 <= kBehzRowsFusedAbove", batch=25, L=3),
        shape("N4096-row-fused", 4096, BITS_TILED_64,
              "behz_rows_fused_supported: items * record_rows = 21 > HEAMD_BEHZ_FUSED_ABOVE = 0, log_degree 12; mul_rows_fused: "
              "batch * L = 9 < 1024: the lift, then every band on the caller's stream", setenv={"HEAMD_BEHZ_FUSED_ABOVE": "0"},
              batch=3, L=3),
        shape("N4096-side-lane-one-part", 4096, BITS_TILED_64,
              "mul_rows_fused: batch * L = 1026 >= 1024: the Q band on the side lane; batch = 342 < 256 * kBehzFloorParts: the floor "
              "in one part (342 * 7 > kBehzRowsFusedAbove)", batch=342, L=3),
        shape("N4096-side-lane-floor-in-parts", 4096, BITS_TILED_64,
              "mul_rows_fused: batch * L = 1024 >= 1024 and batch >= 256 * kBehzFloorParts: the Q band on the side lane, the Bsk "
              "band and the floor in two parts of 512 items (1024 * 3 > kBehzRowsFusedAbove)", batch=1024, L=1),
        shape("N16384", 16384, BITS_TILED, "ntt_policy.hpp kInterleaved16384 / kInterleavedFusedLoads: log_degree 14 runs the "
              "fused loads as interleaved sub-rows; rows_fused_shape false (log_degree not 12 or 13)", batch=2, L=3),
        shape("N4096-L2", 4096, BITS_TILED, BELOW, batch=3, L=2),
    ],
    # ---- relinearize (relinearize_pipeline -> key_switch_pipeline_grouped)
    "he_bfv_relinearize_device": [
        # SMALL: launch_ntt_spread `default: return hipErrorNotSupported` (log_degree < 12): launch_key_switch_spread + ntt_rows,
        #   launch_key_switch_mac + ntt_rows, launch_key_switch_finish
        # TILED: launch_ntt_spread fused; ntt_key_mac_finish_supported false (polys * 2 * (L + 1) = 24 <= 2 kOneGeneration);
        #   launch_key_mac_runs: 24 <= kOneGeneration: one launch; launch_key_switch_finish
        shape("N4096-key-mac-band-runs", 4096, BITS_TILED,
              "launch_key_mac_runs: records * count = 65 * 2 * 4 = 520 > kOneGeneration: one launch per band run; "
              "ntt_key_mac_finish_supported false: 520 <= 2 kOneGeneration", batch=65, L=3),
        shape("N4096-fused-end", 4096, BITS_TILED,
              "ntt_key_mac_finish_supported: polys * 2 * (L + 1) = 129 * 8 = 1032 > 2 kOneGeneration: the q_ks row first, then the "
              "rows r < L with the key switch's last step in their store", batch=129, L=3),
        shape("N4096-in-place", 4096, BITS_TILED,
              "bfv_relinearize: batch == 1 allows out == ct3 (a batch of one is never fused: launch_key_switch_finish)",
              alias=("out", "ct3"), batch=1, L=3),
        shape("N16384", 16384, BITS_TILED, "launch_ntt_spread case 14: interleaved sub-rows; launch_ntt_key_mac_inverse "
              "`kFusedKeyMacAt16384 || log_degree != 14` false: launch_key_switch_mac + ntt_rows", batch=2, L=3),
        shape("N4096-L2", 4096, BITS_TILED, BELOW, batch=3, L=2),
    ],
    # ---- applyGalois (bfv_apply_galois_grouped); 4-byte words always take the rotated copy (`sizeof(W) == 8`)
    "he_bfv_apply_galois_device": [
        # SMALL: galois_switch_fused: launch_ntt_spread not supported -> launch_galois_coeff + key_switch_pipeline_grouped, unfused
        # TILED: `ct != out`: galois_switch_fused, fused_end false (3 * 8 = 24 <= 2 kOneGeneration): key_mac_to_coeff +
        #   launch_galois_finish
        shape("N4096-fused-end", 4096, BITS_TILED,
              "galois_switch_fused (ct != out): ntt_key_mac_finish_supported(smallest_run * group_size = 129): 1032 > 2 "
              "kOneGeneration: launch_ntt_key_mac_inverse_finish", batch=129, L=3),
        shape("N4096-in-place", 4096, BITS_TILED,
              "`ct != out` false: launch_galois_coeff into `rotated`, then key_switch_pipeline_grouped", alias=("out", "ct"),
              batch=3, L=3),
        shape("N4096-in-place-fused-end", 4096, BITS_TILED,
              "out == ct and key_mac_and_finish: 129 * 8 > 2 kOneGeneration", alias=("out", "ct"), batch=129, L=3),
        shape("N16384", 16384, BITS_TILED, "launch_ntt_spread case 14 with a Galois element; ntt_key_mac_finish_supported false at "
              "log_degree 14; launch_ntt_key_mac_inverse not supported: the unfused key MAC, launch_galois_finish", batch=2, L=3),
        shape("N4096-L2", 4096, BITS_TILED, BELOW, batch=3, L=2),
    ],
    "he_bfv_apply_galois_grouped_device": [
        # two groups under two keys: every run of equal keys is one group
        shape("N4096-fused-end", 4096, BITS_TILED_64,
              "galois_switch_fused: smallest_run * group_size = 129: one launch_ntt_key_mac_inverse_finish per run, poly_base = "
              "the run's first item", batch=129, L=3),
        shape("N4096-in-place", 4096, BITS_TILED_64, "out == ct: the rotated copy, one key MAC per run, one finish over the batch",
              alias=("out", "ct"), batch=3, L=3),
        shape("N16384", 16384, BITS_TILED_64, "as he_bfv_apply_galois_device at log_degree 14", batch=2, L=3),
        shape("N4096-L2", 4096, BITS_TILED_64, BELOW, batch=3, L=2),
    ],
    # ---- ct . ct (inner_product_pipeline): lift_pairs_to_eval, launch_tensor_accumulate, drop_extended_base
    "he_bfv_inner_product_device": [
        # SMALL: the lift writes the copy, ntt_records (log_degree < 12)
        # TILED: ntt_lifted_forward_supported false: 3 * 4 * 7 = 84 <= kOneGeneration
        shape("N4096-lift-from-source", 4096, BITS_TILED,
              "ntt_lifted_forward_supported: records * record_rows = 19 * 4 * 7 = 532 > kOneGeneration", count=19, L=3),
        shape("N16384", 16384, BITS_TILED, "interleaved transforms over [Q, Bsk] (log_degree 14)", count=2, L=3),
        shape("N4096-L2", 4096, BITS_TILED, BELOW, count=3, L=2),
    ],
    # ---- Bfv.dotProduct (secret_dot_product): Coeff input goes through a copy in the workspace, Eval input does not
    "he_bfv_secret_dot_product_device": [
        shape("N4096-eval-three-polys", 4096, BITS_TILED, "`is_eval`: one kernel, one inverse transform, no copy; s^2 in registers",
              batch=3, L=3, polys=3, is_eval=1),
        shape("N4096-one-poly", 4096, BITS_TILED, "`!is_eval && poly_count == 1`: the dot product is c0, one copy", batch=3, L=3,
              polys=1),
        shape("N4096-L2", 4096, BITS_TILED, BELOW, batch=3, L=2, polys=3),
    ],
}


def shapes(row):
    return [SMALL, TILED] + FORMS.get(row.name, [])


def words_of(row, shp):
    """The slab words a row runs at under a shape, in bytes"""
    words = (8,) if row.words == 64 else (8, 4)
    return [w for w in words if 8 * w in shp.bits]


def degree_of(row, shp):
    return A.RINGS[row.ring][0] if shp.degree is None else shp.degree


def environment(row, shp, ring_moduli, word_bytes):
    """aliasing_cases.environment at the shape's degree, with the parameters that follow from the ring"""
    overrides = dict(shp.overrides)
    if row.context != "bfv":
        overrides.pop("L", None)
    env = A.environment(row, ring_moduli, word_bytes, overrides)
    env["N"] = degree_of(row, shp)
    for name, expression in DERIVED.get(row.name, {}).items():
        env[name] = int(eval(expression, dict(env)))  # noqa: S307
    return env


def workspace_arguments(row, env):
    """-> (function name, [arguments behind the context]) or None"""
    if row.name not in WORKSPACE:
        return None
    function, arguments = WORKSPACE[row.name]
    return function, [int(eval(token, dict(env))) for token in arguments.split()]  # noqa: S307


def fill_rows(kind, env, ring_moduli, qbsk_moduli):
    """The moduli a residue kind's rows lie under"""
    return {"q": env["q"], "all": list(ring_moduli), "qbsk": qbsk_moduli}[kind]
