"""The pointer contract of include/he_amd.h, entry by entry, in executable form.

Every `*_device` entry of the polynomial, wire-format, RNS, BFV, decrypt and encrypt layers that takes two or more device
slabs has a row here: how it is called, how many bytes each slab spans as a function of the call's arguments (the layouts
the header states: `in = batch L N w`, `out = batch (L - 1) N w`, ...), which slabs the call writes, and which of them may be
exactly the same memory.  The rules the rows are read under (he_amd.h, "Pointer contract"):

  1. slabs a call only reads may be the same memory or overlap freely;
  2. an in-place entry takes its read-only operand at exactly the slab it updates where each lane reads only the words it
     writes (`same` below); any other overlap of the two is HE_ERR_INVALID_ARGUMENT;
  3. an out-of-place entry refuses every byte-range overlap between a slab it writes (a caller's workspace included) and any
     other slab of the call, but for the exceptions named in `same`;
  4. abutting ranges do not overlap, and empty ranges (a batch of 0) overlap nothing.

Nothing here imports the device package or reads the C++ (invoke() is handed the loaded library): tests/test_aliasing_contract.py (host-only contexts, fake
addresses) and tests/test_gpu_aliasing.py (the 4-byte forms, on a device) hold the library to this table, and the former
holds the table to the header's prototypes.

Sizes are Python expressions over the row's parameters:
  N degree, L the call's moduli_count, TOP the context's ciphertext moduli count, ALL its coefficient moduli count, w the
  slab word in bytes, q the context's moduli (the ciphertext level's for a scheme context), plus the row's own arguments.
"""
import collections
import ctypes

# ---- the rings the rows are laid out over -----------------------------------------------------------------------------------
# Moduli below 2^30, so that one parameter set serves both slab words.  (degree, bits of the coefficient moduli)
RINGS = {
    "small": (8, (27, 28, 28)),    # a polynomial context over all three; a scheme context with TOP = 2 and a key-switching modulus
    "packed": (256, (27, 28, 28)),  # the packed-plaintext layout needs N >= 256
}
PLAINTEXT_BITS = 17

Case = collections.namedtuple("Case", "name context words args slabs written same says params ring zero")


def case(name, context, words, args, slabs, written, same=(), says=None, params=None, ring="small", zero="batch"):
    """name     the 8-byte entry (or the only one)
    context  "poly" (he_poly_context), "bfv" (he_bfv_context) or None (no context argument)
    words    "twin": the entry has a `_u32` twin; "arg": it takes word_bits as an argument; 64: 8-byte slabs only
    args     the C arguments behind the context and before the stream: names of slabs, of parameters, or literals
    slabs    {argument: bytes expression}, device slabs only
    written  the slabs the call writes
    same     [(a, b, {parameter overrides})]: a and b may start at the same byte under those parameters
    says     {argument: the name the error text uses} where it differs
    zero     the parameter that makes the call empty (None: the entry has none)"""
    defaults = dict(batch=3, polys=2, count=3, columns=2, items=2, keys=2, skip=0, workspace_bytes=4096, is_eval=0, eval_out=0,
                    element=3, power=1, factor=1, words=24, L=2, stride=0, non_temporal=0)
    defaults.update(params or {})
    return Case(name, context, words, args.split(), collections.OrderedDict(slabs), tuple(written.split()), tuple(same),
                says or {}, defaults, ring, zero)


POLY = "batch*L*N*w"
CT = "batch*polys*L*N*w"
KEY = "TOP*2*(TOP+1)*N*w"  # a key-switching key: TOP ciphertexts over the TOP + 1 moduli of the key-switching context
RECORD = "sum((N*(qi.bit_length()-skip)+7)//8 for qi in q)"  # PolyRq.serialize of one polynomial
PACKED = "sum(N//64*qi.bit_length() for qi in q)*8"           # one packed plaintext

CASES = [
    # ---- polynomial layer (in place on lhs / data)
    case("he_poly_add_device", "poly", "twin", "lhs rhs batch", {"lhs": POLY, "rhs": POLY}, "lhs", same=[("lhs", "rhs", {})]),
    case("he_poly_sub_device", "poly", "twin", "lhs rhs batch", {"lhs": POLY, "rhs": POLY}, "lhs", same=[("lhs", "rhs", {})]),
    case("he_poly_mul_device", "poly", "twin", "lhs rhs batch", {"lhs": POLY, "rhs": POLY}, "lhs", same=[("lhs", "rhs", {})]),
    case("he_poly_divide_and_round_q_last_device", "poly", "twin", "in out batch",
         {"in": POLY, "out": "batch*(L-1)*N*w"}, "out"),
    case("he_poly_adding_lazy_product_device", "poly", 64, "lhs rhs acc_lo_hi",
         {"lhs": "L*N*8", "rhs": "L*N*8", "acc_lo_hi": "L*N*16"}, "acc_lo_hi", zero=None),
    case("he_poly_reduce_accumulator_device", "poly", 64, "acc_lo_hi out", {"acc_lo_hi": "L*N*16", "out": "L*N*8"}, "out",
         zero=None),
    case("he_poly_apply_galois_device", "poly", 64, "in out batch element 0", {"in": POLY, "out": POLY}, "out"),
    case("he_poly_multiply_power_of_x_device", "poly", 64, "in out batch power", {"in": POLY, "out": POLY}, "out"),
    # ---- wire format
    case("he_poly_serialize_device", "poly", "twin", "device_slab batch skip device_bytes",
         {"device_slab": POLY, "device_bytes": "batch*(%s)" % RECORD}, "device_bytes"),
    case("he_poly_deserialize_device", "poly", "twin", "device_bytes bytes_per_poly batch skip device_slab",
         {"device_bytes": "batch*bytes_per_poly", "device_slab": POLY}, "device_slab", params={"bytes_per_poly": 96}),
    case("he_poly_random_from_seeds_device", "poly", "twin", "device_seeds batch device_slab",
         {"device_seeds": "batch*32", "device_slab": POLY}, "device_slab"),
    case("he_ciphertexts_serialize_device", "poly", "twin", "cts count polys None records stride",
         {"cts": "count*polys*L*N*w", "records": "(count-1)*stride+2+polys*(%s)" % RECORD}, "records",
         params={"stride": 200}, zero="count"),
    case("he_ciphertexts_deserialize_device", "poly", "twin", "records stride count polys None cts device_header_mismatch",
         {"records": "(count-1)*stride+2+polys*(%s)" % RECORD, "cts": "count*polys*L*N*w", "device_header_mismatch": "4"},
         "cts device_header_mismatch", params={"stride": 200}, zero="count"),
    case("he_ciphertexts_deserialize_seeded_device", "poly", "twin", "poly0_bytes stride seeds count 0 cts",
         {"poly0_bytes": "(count-1)*stride+(%s)" % RECORD, "seeds": "count*32", "cts": "count*2*L*N*w"}, "cts",
         params={"stride": 96}, zero="count"),
    # ---- the word-size bridge (no context: on a device only the refused forms are called with addresses that are not memory)
    case("he_words_widen_u32_device", None, 64, "device_in device_out words", {"device_in": "words*4", "device_out": "words*8"},
         "device_out", zero="words"),
    case("he_words_narrow_u64_device", None, 64, "device_in device_out words", {"device_in": "words*8", "device_out": "words*4"},
         "device_out", zero="words"),
    case("he_words_copy_device", None, 64, "device_in device_out words non_temporal",
         {"device_in": "words*8", "device_out": "words*8"}, "device_out", zero="words"),
    # ---- RNS tool
    case("he_rns_lift_q_to_qbsk_device", "bfv", "twin", "L in out batch", {"in": POLY, "out": "batch*(2*L+1)*N*w"}, "out"),
    case("he_rns_floor_qbsk_to_q_device", "bfv", "twin", "L in out batch", {"in": "batch*(2*L+1)*N*w", "out": POLY}, "out"),
    case("he_rns_scale_and_round_device", "bfv", "twin", "L in factor out batch", {"in": POLY, "out": "batch*N*w"}, "out"),
    # ---- BFV
    case("he_bfv_mul_device", "bfv", "twin", "L lhs rhs out batch workspace workspace_bytes",
         {"lhs": "batch*2*L*N*w", "rhs": "batch*2*L*N*w", "out": "batch*3*L*N*w", "workspace": "workspace_bytes"},
         "out workspace"),
    case("he_bfv_relinearize_device", "bfv", "twin", "L ct3 key out batch workspace workspace_bytes",
         {"ct3": "batch*3*L*N*w", "key": KEY, "out": "batch*2*L*N*w", "workspace": "workspace_bytes"}, "out workspace",
         same=[("out", "ct3", {"batch": 1})]),
    case("he_bfv_apply_galois_device", "bfv", "twin", "L ct element galois_key out batch workspace workspace_bytes",
         {"ct": "batch*2*L*N*w", "galois_key": KEY, "out": "batch*2*L*N*w", "workspace": "workspace_bytes"}, "out workspace",
         same=[("out", "ct", {})]),
    case("he_bfv_apply_galois_grouped_device", "bfv", 64,
         "L ct element galois_keys[] 2 batch out workspace workspace_bytes",
         {"ct": "2*batch*2*L*N*w", "galois_keys[0]": KEY, "galois_keys[1]": KEY, "out": "2*batch*2*L*N*w",
          "workspace": "workspace_bytes"}, "out workspace", same=[("out", "ct", {})],
         says={"galois_keys[0]": "galois_key", "galois_keys[1]": "galois_key"}),
    case("he_bfv_mod_switch_down_device", "bfv", "twin", "L polys in out batch", {"in": CT, "out": "batch*polys*(L-1)*N*w"},
         "out"),
    case("he_bfv_mod_switch_down_to_single_device", "bfv", 64, "L polys in out batch", {"in": CT, "out": "batch*polys*N*w"},
         "out", same=[("out", "in", {"L": 1})]),
    case("he_bfv_mul_plain_device", "bfv", "twin", "L polys ct pt batch", {"ct": CT, "pt": POLY}, "ct",
         same=[("ct", "pt", {"batch": 1}), ("ct", "pt", {"polys": 1})]),
    case("he_bfv_add_plain_device", "bfv", "twin", "L polys ct plaintexts batch", {"ct": CT, "plaintexts": "batch*N*w"}, "ct"),
    case("he_bfv_sub_plain_device", "bfv", "twin", "L polys ct plaintexts batch", {"ct": CT, "plaintexts": "batch*N*w"}, "ct"),
    case("he_bfv_inner_product_plain_device", "bfv", 64, "L polys cts pts None count columns out",
         {"cts": "count*polys*L*N*w", "pts": "columns*count*L*N*w", "out": "columns*polys*L*N*w"}, "out", zero="columns"),
    case("he_bfv_inner_product_plain_resident_device", "bfv", "twin", "L polys cts pts present_device count columns out",
         {"cts": "count*polys*L*N*w", "pts": "columns*count*L*N*w", "present_device": "columns*count",
          "out": "columns*polys*L*N*w"}, "out", zero="columns"),
    case("he_bfv_pack_plaintexts_device", "bfv", 64, "L plaintexts_eval count packed",
         {"plaintexts_eval": "count*L*N*8", "packed": "count*(%s)" % PACKED}, "packed", ring="packed", zero="count"),
    case("he_bfv_inner_product_plain_packed_device", "bfv", 64, "L polys cts packed_pts present_device count columns out",
         {"cts": "count*polys*L*N*w", "packed_pts": "columns*count*(%s)" % PACKED, "present_device": "columns*count",
          "out": "columns*polys*L*N*w"}, "out", says={"packed_pts": "pts"}, ring="packed", zero="columns"),
    case("he_bfv_inner_product_device", "bfv", "twin", "L lhs rhs count out workspace workspace_bytes",
         {"lhs": "count*2*L*N*w", "rhs": "count*2*L*N*w", "out": "3*L*N*w", "workspace": "workspace_bytes"}, "out workspace",
         zero=None),
    case("he_bfv_inner_product_shared_device", "bfv", "twin", "L lhs rhs count items out",
         {"lhs": "count*2*L*N*w", "rhs": "items*count*2*L*N*w", "out": "items*3*L*N*w"}, "out", zero="items"),
    case("he_bfv_plaintext_to_eval_device", "bfv", "twin", "L plaintext out batch", {"plaintext": "batch*N*w", "out": POLY},
         "out"),
    case("he_bfv_plaintext_to_coeff_device", "bfv", "twin", "L plaintext_eval out batch",
         {"plaintext_eval": POLY, "out": "batch*N*w"}, "out"),
    # ---- decryption (the slab word is an argument; the first L rows of the secret key are read)
    case("he_bfv_secret_dot_product_device", "bfv", "arg",
         "word_bits L polys is_eval cts secret_key out batch workspace workspace_bytes",
         {"cts": CT, "secret_key": "L*N*w", "out": POLY, "workspace": "workspace_bytes"}, "out workspace"),
    case("he_bfv_decrypt_device", "bfv", "arg",
         "word_bits L polys is_eval cts secret_key factor out_plaintexts batch workspace workspace_bytes",
         {"cts": CT, "secret_key": "L*N*w", "out_plaintexts": "batch*N*w", "workspace": "workspace_bytes"},
         "out_plaintexts workspace"),
    case("he_bfv_noise_norm_device", "bfv", "arg",
         "word_bits L polys is_eval cts secret_key out_limbs batch workspace workspace_bytes",
         {"cts": CT, "secret_key": "L*N*w", "out_limbs": "batch*LIMBS*8", "workspace": "workspace_bytes"},
         "out_limbs workspace"),
    case("he_bfv_is_transparent_device", "bfv", "arg", "word_bits L polys cts out_flags batch",
         {"cts": CT, "out_flags": "batch"}, "out_flags"),
    # ---- secret keys, encryption, evaluation keys (the slab word is an argument)
    case("he_bfv_generate_secret_key_device", "bfv", "arg", "word_bits seeds out batch workspace workspace_bytes",
         {"seeds": "batch*32", "out": "batch*ALL*N*w", "workspace": "workspace_bytes"}, "out workspace"),
    case("he_bfv_encrypt_zero_device", "bfv", "arg",
         "word_bits L eval_out secret_key a_seeds error_seeds out batch workspace workspace_bytes",
         {"secret_key": "L*N*w", "a_seeds": "batch*32", "error_seeds": "batch*32", "out": "batch*2*L*N*w",
          "workspace": "workspace_bytes"}, "out workspace"),
    case("he_bfv_encrypt_device", "bfv", "arg",
         "word_bits L secret_key a_seeds error_seeds plaintexts out batch workspace workspace_bytes",
         {"secret_key": "L*N*w", "a_seeds": "batch*32", "error_seeds": "batch*32", "plaintexts": "batch*N*w",
          "out": "batch*2*L*N*w", "workspace": "workspace_bytes"}, "out workspace"),
    case("he_bfv_generate_key_switch_keys_device", "bfv", "arg",
         "word_bits secret_key current_keys a_seeds error_seeds out keys workspace workspace_bytes",
         {"secret_key": "ALL*N*w", "current_keys": "keys*ALL*N*w", "a_seeds": "keys*TOP*32", "error_seeds": "keys*TOP*32",
          "out": "keys*(%s)" % KEY, "workspace": "workspace_bytes"}, "out workspace", zero="keys"),
    case("he_bfv_generate_relinearization_key_device", "bfv", "arg",
         "word_bits secret_key a_seeds error_seeds out workspace workspace_bytes",
         {"secret_key": "ALL*N*w", "a_seeds": "TOP*32", "error_seeds": "TOP*32", "out": KEY, "workspace": "workspace_bytes"},
         "out workspace", zero=None),
    case("he_bfv_generate_galois_keys_device", "bfv", "arg",
         "word_bits secret_key elements[] count a_seeds error_seeds out workspace workspace_bytes",
         {"secret_key": "ALL*N*w", "a_seeds": "count*TOP*32", "error_seeds": "count*TOP*32", "out": "count*(%s)" % KEY,
          "workspace": "workspace_bytes"}, "out workspace", zero="count"),
    case("he_poly_random_ternary_from_seeds_device", "poly", "arg", "word_bits seeds batch out",
         {"seeds": "batch*32", "out": POLY}, "out"),
    case("he_poly_random_centered_binomial_from_seeds_device", "poly", "arg", "word_bits seeds batch out",
         {"seeds": "batch*32", "out": POLY}, "out"),
]

# One device slab and a HOST array: nothing to alias.
HOST_OPERAND = {
    "he_poly_mul_scalar_device": "scalar_residues is a host array",
}

# Entries whose pointers are all host memory, or a host and a device side of one copy (no two device slabs).
HOST_ONLY = {
    "he_memcpy_h2d": "one side is host memory",
    "he_memcpy_d2h": "one side is host memory",
    "he_generate_primes": "host arrays",
    "he_poly_divide_and_round_q_last": "host slabs, staged through buffers of the library's own",
    "he_poly_context_copy_ntt_tables": "host arrays",
    "he_ciphertexts_wire_plan": "host words",
    "he_bfv_noise_budget_from_norm": "host words",
    "he_shard_bounds": "host words",
}

# The composite protocol entries: each is a pipeline of the entries above over scratch of its own; what may alias among
# their arguments is a later change.  By prefix or suffix of the entry's name.
DEFERRED = {
    "he_pir_": "PIR responses, expansion, database processing and database files (the file entries already refuse overlaps)",
    "he_pnns_": "PNNS matrices and responses",
    "he_simple_pir_": "SimplePIR databases and responses",
    "he_keyword_": "keyword PIR tables, buckets and sharding",
    "_group": "multi-device forms of the entries above",
}


def deferred_reason(name):
    for mark, reason in DEFERRED.items():
        if name.startswith(mark) or name.endswith(mark):
            return reason
    return None


def entry_names(row):
    """The C entries of a row: the 8-byte one and its twin."""
    return [row.name, row.name + "_u32"] if row.words == "twin" else [row.name]


def limbs(moduli):
    product = 1
    for m in moduli:
        product *= m
    return (product.bit_length() + 63) // 64


def environment(row, ring_moduli, word_bytes, overrides=None):
    """The names a row's size expressions are evaluated over: ring_moduli are the coefficient moduli of the row's ring (a
    polynomial context holds them all, a scheme context all but the last at its top level)."""
    degree = RINGS[row.ring][0]
    env = dict(row.params)
    env.update(overrides or {})
    if row.context == "bfv":
        top = len(ring_moduli) - 1
        env.update(TOP=top, ALL=len(ring_moduli), q=list(ring_moduli[:env["L"]]), LIMBS=limbs(ring_moduli[:env["L"]]))
    else:
        env.update(L=len(ring_moduli), q=list(ring_moduli))
    env.update(N=degree, w=word_bytes, word_bits=8 * word_bytes)
    return env


def slab_bytes(row, env):
    return collections.OrderedDict((name, int(eval(expr, dict(env)))) for name, expr in row.slabs.items())  # noqa: S307


def pairs(row):
    """Every (written slab, other slab) of a row, each unordered pair once."""
    seen, out = set(), []
    for a in row.written:
        for b in row.slabs:
            if a != b and frozenset((a, b)) not in seen:
                seen.add(frozenset((a, b)))
                out.append((a, b))
    return out


def may_be_same(row, a, b, overrides):
    """Whether a and b may start at the same byte under a row's defaults changed by `overrides`."""
    return any({x, y} == {a, b} and all(overrides.get(k, row.params.get(k)) == v for k, v in need.items())
               for x, y, need in row.same)


def overlap_positions(read_at, read_bytes, written_bytes):
    """Where a written slab overlaps a read one: the same first byte, its first byte on the other's last, its last byte on the
    other's first; and the two positions at which they abut."""
    refused = {"same": read_at, "first on last": read_at + read_bytes - 1, "last on first": read_at - written_bytes + 1}
    accepted = {"behind": read_at + read_bytes, "before": read_at - written_bytes}
    return refused, accepted


def invoke(lib, row, name, handle, env, where):
    """Calls the entry `name` of a row (its 8-byte name or its twin's) on the loaded library `lib` with the row's slabs at the
    addresses of `where`, the other arguments from `env`, a null stream -> (status, last-error text)."""
    fn = getattr(lib, name)
    args, keep = [], []
    for token in row.args:
        if token in row.slabs:
            args.append(ctypes.c_void_p(where[token]))
        elif token == "galois_keys[]":  # a host array of device pointers
            keys = (ctypes.c_void_p * 2)(where["galois_keys[0]"], where["galois_keys[1]"])
            keep.append(keys)
            args.append(ctypes.cast(keys, fn.argtypes[len(args) + (row.context is not None)]))
        elif token == "elements[]":  # a host array of Galois elements, valid for N >= 4
            elements = (ctypes.c_uint64 * max(env["count"], 1))(*[3, 5, 7][:env["count"]])
            keep.append(elements)
            args.append(elements)
        elif token == "None":
            args.append(None)
        elif token in env:
            args.append(env[token])
        else:
            args.append(int(token))
    head = [handle] if row.context is not None else []
    status = fn(*head, *args, None)
    return status, lib.he_last_error_message().decode()
