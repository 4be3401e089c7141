"""What every device method of heamd hands to C, without a device or a built library (binding_recorder.py): the entry it
reaches, the arguments in order (a pointer as the name of the tensor it points into, NULL as None, integers and ctypes arrays
by value) and the dtype and shape of what it returns, for both slab words, N = 8, L = 2, batch 3, with the optional arguments
both left out and given.  binding_call_shapes.json holds the records of the binding before its methods were written once over
a word descriptor; `python tests/test_binding_call_shapes.py` writes the file anew from the binding it finds.

Every public device method of PolyContext, BfvContext / BfvContext32, SimplePirServer / SimplePirServer32 and PnnsContext is
driven; none is left out.  (Host-only methods -- the *_host forms, shapes, plans, byte counts, workspace sizes, sub-contexts --
reach no device entry and are not part of the table.)  relinearize and apply_galois of BfvContext32 are driven with a key
only: without one the earlier binding raised AttributeError where it now passes NULL, as BfvContext does."""
import ctypes
import json
import os

import torch

from binding_recorder import BATCH, DEGREE, MODULI, Stream, recording

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "binding_call_shapes.json")
N, L, B = DEGREE, MODULI, BATCH
I64, I32, U8 = torch.int64, torch.int32, torch.uint8


def drive(heamd, rec):
    """every case -> {"calls": [[entry, arguments], ...], "returns": ...}"""
    table, stream, t = {}, Stream(), rec.tensor

    def case(name, call, host_len=0):
        assert name not in table, name
        rec.calls.clear()
        rec.made, rec.host_len = 0, host_len
        value = call()
        table[name] = {"calls": [list(c) for c in rec.calls], "returns": rec.result(value)}
        return value

    # ---- PolyContext
    poly = case("PolyContext()", lambda: heamd.PolyContext(N, [97, 193]), host_len=L)
    for tag, dt, sfx in (("64", I64, ""), ("32", I32, "_u32")):
        slab = lambda name="slab": t(name, (B, L, N), dt)  # noqa: E731
        if dt is I64:
            case("poly.forward_ntt_", lambda: poly.forward_ntt_(slab(), stream))
            case("poly.inverse_ntt_", lambda: poly.inverse_ntt_(slab(), stream=stream))
            case("poly.ntt_variant_", lambda: poly.ntt_variant_(slab(), True, 2, stream))
            case("poly.forward_ntt_rows_", lambda: poly.forward_ntt_rows_(97, t("rows", (5, N), dt), stream))
            case("poly.inverse_ntt_rows_", lambda: poly.inverse_ntt_rows_(193, t("rows", (5, N), dt), stream))
            case("poly.add_", lambda: poly.add_(slab("lhs"), slab("rhs"), stream))
            case("poly.sub_", lambda: poly.sub_(slab("lhs"), slab("rhs"), stream))
            case("poly.mul_", lambda: poly.mul_(slab("lhs"), slab("rhs"), stream))
            case("poly.neg_", lambda: poly.neg_(slab(), stream))
            case("poly.mul_scalar_", lambda: poly.mul_scalar_(slab(), [5, 1 << 40], stream), host_len=L)
            case("poly.divide_and_round_q_last", lambda: poly.divide_and_round_q_last(slab(), stream))
            case("poly.random_from_seeds", lambda: poly.random_from_seeds(t("seeds", (B, 32), U8), stream))
            case("poly.serialize", lambda: poly.serialize(slab(), 0, stream))
            case("poly.serialize skip", lambda: poly.serialize(slab(), skip_lsbs=3, stream=stream))
            case("poly.deserialize", lambda: poly.deserialize(t("data", (B, 40), U8), 2, stream))
            case("poly.apply_galois", lambda: poly.apply_galois(slab(), 3, True, stream))
            case("poly.multiply_power_of_x", lambda: poly.multiply_power_of_x(slab(), -5, stream))
            case("poly.adding_lazy_product_", lambda: poly.adding_lazy_product_(
                t("lhs", (L, N), dt), t("rhs", (L, N), dt), t("acc", (L, 2 * N), dt), stream))
            case("poly.reduce_accumulator", lambda: poly.reduce_accumulator(t("acc", (L, 2 * N), dt), stream))
        else:
            case("poly.forward_ntt_u32_", lambda: poly.forward_ntt_u32_(slab(), stream))
            case("poly.inverse_ntt_u32_", lambda: poly.inverse_ntt_u32_(slab(), stream=stream))
            for op in ("add", "sub", "mul"):
                case(f"poly.elementwise_u32_ {op}", lambda: poly.elementwise_u32_(op, slab("lhs"), slab("rhs"), stream))
            case("poly.elementwise_u32_ neg", lambda: poly.elementwise_u32_("neg", slab("lhs"), stream=stream))
            case("poly.mul_scalar_u32_", lambda: poly.mul_scalar_u32_(slab(), [5, (1 << 32) - 1], stream))
            case("poly.divide_and_round_q_last_u32", lambda: poly.divide_and_round_q_last_u32(slab(), stream))
            case("poly.random_from_seeds_u32", lambda: poly.random_from_seeds_u32(t("seeds", (B, 32), U8), stream))
            case("poly.serialize_u32", lambda: poly.serialize_u32(slab(), 0, stream))
            case("poly.serialize_u32 skip", lambda: poly.serialize_u32(slab(), skip_lsbs=3, stream=stream))
            case("poly.deserialize_u32", lambda: poly.deserialize_u32(t("data", (B, 40), U8), 2, stream))
        # the methods that take either word
        cts = lambda: t("cts", (B, 2, L, N), dt)  # noqa: E731
        case(f"poly.ciphertexts_serialize {tag}", lambda: poly.ciphertexts_serialize(cts(), stream=stream))
        case(f"poly.ciphertexts_serialize {tag} given", lambda: poly.ciphertexts_serialize(
            cts(), skip_lsbs=[4, 7], record_stride=96, out=t("out", (B * 96 + 8,), U8), stream=stream))
        bits = int(tag)
        case(f"poly.ciphertexts_deserialize {tag}", lambda: poly.ciphertexts_deserialize(
            t("records", (B, 90), U8), B, 2, word_bits=bits, stream=stream))
        case(f"poly.ciphertexts_deserialize {tag} given", lambda: poly.ciphertexts_deserialize(
            t("records", (B, 96), U8), B, 2, skip_lsbs=[4, 7], record_stride=96, word_bits=bits, out=cts(),
            mismatch=t("mismatch", (1,), I32), stream=stream))
        case(f"poly.ciphertexts_deserialize_seeded {tag}", lambda: poly.ciphertexts_deserialize_seeded(
            t("poly0", (B, 40), U8), t("seeds", (B, 32), U8), B, True, word_bits=bits, stream=stream))
        case(f"poly.ciphertexts_deserialize_seeded {tag} no seeds", lambda: poly.ciphertexts_deserialize_seeded(
            t("poly0", (B, 48), U8), None, B, False, record_stride=48, word_bits=bits, stream=stream))
        case(f"poly.ciphertexts_deserialize_seeded {tag} no poly0", lambda: poly.ciphertexts_deserialize_seeded(
            None, t("seeds", (B, 32), U8), B, False, word_bits=bits, out=cts(), stream=stream))

    # ---- BfvContext / BfvContext32: `dt` is the class's slab word; entries without a 4-byte twin take int64 in both
    contexts = {}
    for name, make in (("BfvContext", lambda: heamd.BfvContext(N, 17, [97, 193, 257])),
                       ("BfvContext32", lambda: heamd.BfvContext32(N, 17, [97, 193, 257])),
                       ("BfvContext word_bits=32", lambda: heamd.BfvContext(N, 17, [97, 193, 257], word_bits=32)),
                       ("BfvContext host_only", lambda: heamd.BfvContext(N, 17, [97, 193, 257], host_only=True)),
                       ("BfvContext host_only word_bits=32",
                        lambda: heamd.BfvContext(N, 17, [97, 193, 257], host_only=True, word_bits=32)),
                       ("BfvContext32 host_only", lambda: heamd.BfvContext32(N, 17, [97, 193, 257], host_only=True))):
        contexts[name] = case(f"{name}()", make, host_len=3)
    dims = [2, 3]
    for name in ("BfvContext", "BfvContext32", "BfvContext word_bits=32"):
        bfv = contexts[name]
        dt = I32 if name == "BfvContext32" else I64
        ct = lambda label="ct", polys=2, d=dt: t(label, (B, polys, L, N), d)  # noqa: E731
        key = lambda label="key", d=dt: t(label, (L, 2, L + 1, N), d)  # noqa: E731
        mask = lambda shape, label="mask": t(label, shape, U8)  # noqa: E731
        workspace = lambda: t("workspace", (64,), U8)  # noqa: E731
        dim0 = lambda d=dt: t("dim0", (2, 2, L, N), d)  # noqa: E731
        rest = lambda d=dt: t("rest", (3, 2, L, N), d)  # noqa: E731
        galois = lambda: {5: t("galois5", (4, N), I64), 3: t("galois3", (4, N), I64)}  # noqa: E731
        c = lambda method, call, host_len=0, n=name: case(f"{n}.{method}", call, host_len)  # noqa: E731

        c("lift_q_to_qbsk", lambda: bfv.lift_q_to_qbsk(t("polys", (B, L, N), dt), stream=stream))
        c("lift_q_to_qbsk L=1", lambda: bfv.lift_q_to_qbsk(t("polys", (B, 1, N), dt), 1, stream))
        c("floor_qbsk_to_q", lambda: bfv.floor_qbsk_to_q(t("polys", (B, 2 * L + 1, N), dt), stream=stream))
        c("mul", lambda: bfv.mul(ct("lhs"), ct("rhs"), stream=stream))
        c("mul workspace", lambda: bfv.mul(ct("lhs"), ct("rhs"), None, stream, workspace()))
        c("relinearize", lambda: bfv.relinearize(ct("ct3", 3), key(), stream=stream))
        c("relinearize workspace", lambda: bfv.relinearize(ct("ct3", 3), key(), None, stream, workspace()))
        c("apply_galois", lambda: bfv.apply_galois(ct(), 3, key(), stream=stream))
        c("apply_galois workspace", lambda: bfv.apply_galois(ct(), 3, key(), None, stream, workspace()))
        if dt is I64:
            c("relinearize no key", lambda: bfv.relinearize(ct("ct3", 3), None, stream=stream))
            c("apply_galois no key", lambda: bfv.apply_galois(ct(), 3, None, stream=stream))
        c("scale_and_round", lambda: bfv.scale_and_round(t("poly", (B, L, N), dt), 4, stream=stream))
        c("plaintext_to_eval", lambda: bfv.plaintext_to_eval(t("plaintext", (B, N), dt), stream=stream))
        c("plaintext_to_coeff", lambda: bfv.plaintext_to_coeff(t("plaintext", (B, L, N), dt), stream=stream))
        c("mod_switch_down", lambda: bfv.mod_switch_down(ct("ct", 3), 3, stream=stream))
        c("mul_plain_", lambda: bfv.mul_plain_(ct(), t("pt", (B, L, N), dt), 2, stream=stream))
        c("add_plain_", lambda: bfv.add_plain_(ct(), t("plaintexts", (B, N), dt), stream=stream))
        c("add_plain_ subtract", lambda: bfv.add_plain_(ct("ct", 3), t("plaintexts", (B, N), dt), 3, True, stream=stream))
        c("inner_product_plain_resident", lambda: bfv.inner_product_plain_resident(
            ct("cts"), t("pts", (2, B, L, N), dt), columns=2, stream=stream))
        c("inner_product_plain_resident mask", lambda: bfv.inner_product_plain_resident(
            ct("cts"), t("pts", (2, B, L, N), dt), mask((2, B)), 2, 2, None, stream))
        c("inner_product", lambda: bfv.inner_product(ct("lhs"), ct("rhs"), stream=stream))
        c("inner_product_shared", lambda: bfv.inner_product_shared(ct("lhs"), t("rhs", (2, B, 2, L, N), dt), stream=stream))
        database = lambda d=dt: t("database", (2, 6, L, N), d)  # noqa: E731
        c("pir_compute_response", lambda: bfv.pir_compute_response(dims, dim0(), None, database(), 2, stream=stream))
        c("pir_compute_response given", lambda: bfv.pir_compute_response(
            dims, dim0(), rest(), database(), 2, mask((2, 6)), key("relin"), stream))
        c("pir_compute_response_queries", lambda: bfv.pir_compute_response_queries(
            dims, t("dim0", (2, 2, 2, L, N), dt), None, database(), 2, None, stream=stream))
        c("pir_compute_response_queries given", lambda: bfv.pir_compute_response_queries(
            dims, t("dim0", (2, 2, 2, L, N), dt), t("rest", (2, 3, 2, L, N), dt), database(), 2,
            [key("relin0"), key("relin1")], mask((2, 6)), stream))
        c("pir_compute_response_to_query", lambda: bfv.pir_compute_response_to_query(
            dims, ct("query"), 2, galois(), None, database(), 2, stream=stream), host_len=2)
        c("pir_compute_response_to_query given", lambda: bfv.pir_compute_response_to_query(
            dims, ct("query"), 2, galois(), key("relin"), [database(), t("database1", (2, 6, L, N), dt)], 2,
            [mask((2, 6)), None], stream), host_len=2)
        c("pir_compute_response_to_query one mask", lambda: bfv.pir_compute_response_to_query(
            dims, ct("query"), 2, {}, key("relin"), database(), 2, mask((2, 6)), stream))
        entries = lambda: t("entries", (4, 5), U8)  # noqa: E731
        c("pir_process_database", lambda: bfv.pir_process_database(entries(), dims, 5, stream=stream))
        c("pir_process_database given", lambda: bfv.pir_process_database(
            entries(), dims, 5, True, [5, 4, 3, 2], 4, (database(), mask((2, 6), "present")), stream=stream), host_len=4)
        c("load_database_segment", lambda: bfv.load_database_segment(
            t("records", (30,), U8), mask((3,), "present"), stream=stream))
        c("load_database_segment given", lambda: bfv.load_database_segment(
            t("records", (40,), U8), mask((3,), "present"), 30, t("out", (3, L, N), dt), t("mismatch", (1,), I32), stream))
        present = lambda: mask((3,), "present").fill_(1)  # noqa: E731
        c("save_database_segment", lambda: bfv.save_database_segment(t("database", (3, L, N), dt), present(), stream=stream))
        c("save_database_segment given", lambda: bfv.save_database_segment(
            t("database", (3, L, N), dt), present(), 100, t("out", (128,), U8), t("mismatch", (1,), I32), stream))
        c("load_database_file", lambda: bfv.load_database_file(bytes([1, 3, 0, 0, 0]) + bytes(30), device="cpu", stream=stream))
        c("save_database_file", lambda: bfv.save_database_file(t("database", (3, L, N), dt), present(), stream))
        # no 4-byte twin: 8-byte slabs in every class
        wide = lambda label="ct", polys=2: ct(label, polys, I64)  # noqa: E731
        c("pir_expand", lambda: bfv.pir_expand(wide("cts"), 4, galois(), stream), host_len=2)
        c("pir_expand_batch", lambda: bfv.pir_expand_batch(t("cts", (2, 1, 2, L, N), I64), 4, [galois(), galois()], stream),
          host_len=2)
        c("pir_compute_response_chunk", lambda: bfv.pir_compute_response_chunk(
            dims, dim0(I64), None, t("database", (6, L, N), I64), stream=stream))
        c("pir_compute_response_chunk given", lambda: bfv.pir_compute_response_chunk(
            dims, dim0(I64), rest(I64), t("database", (6, L, N), I64), [1, 0, 1, 1, 0, 1], key("relin", I64), stream), host_len=6)
        c("pir_dim0_columns", lambda: bfv.pir_dim0_columns(dim0(I64), t("database", (3, 2, L, N), I64), stream=stream))
        c("pir_dim0_columns mask", lambda: bfv.pir_dim0_columns(
            dim0(I64), t("database", (3, 2, L, N), I64), mask((3, 2)), stream))
        c("pir_remaining_dimensions", lambda: bfv.pir_remaining_dimensions(dims, wide("intermediate"), None, stream=stream))
        c("pir_remaining_dimensions given", lambda: bfv.pir_remaining_dimensions(
            dims, wide("intermediate"), rest(I64), key("relin", I64), stream))
        c("mod_switch_down_to_single", lambda: bfv.mod_switch_down_to_single(wide(), 2, stream=stream))
        c("inner_product_plain", lambda: bfv.inner_product_plain(
            wide("cts"), t("pts", (2, B, L, N), I64), columns=2, stream=stream))
        c("inner_product_plain present", lambda: bfv.inner_product_plain(
            wide("cts"), t("pts", (2, B, L, N), I64), [[1, 0, 1], [0, 1, 1]], 2, 2, None, stream), host_len=6)
        c("pack_plaintexts", lambda: bfv.pack_plaintexts(t("plaintexts", (B, L, N), I64), stream=stream))
        c("inner_product_plain_packed", lambda: bfv.inner_product_plain_packed(
            wide("cts"), t("packed", (2 * B * 5 + 1,), I64), columns=2, stream=stream))
        c("inner_product_plain_packed mask", lambda: bfv.inner_product_plain_packed(
            wide("cts"), t("packed", (2 * B * 5 + 1,), I64), mask((2, B)), 2, 2, None, stream))
        c("pir_compute_response_packed", lambda: bfv.pir_compute_response_packed(
            dims, dim0(I64), None, t("packed", (61,), I64), 2, stream=stream))
        c("pir_compute_response_packed given", lambda: bfv.pir_compute_response_packed(
            dims, dim0(I64), rest(I64), t("packed", (61,), I64), 2, mask((2, 6)), key("relin", I64), stream))

        # ---- PnnsContext: its word follows bfv.word_bits
        dt = I64 if name == "BfvContext" else I32
        pnns = case(f"PnnsContext({name})", lambda: heamd.PnnsContext(bfv))
        c = lambda method, call, n=name: case(f"PnnsContext({n}).{method}", call)  # noqa: E731
        vectors = lambda: t("vectors", (3, 4), torch.float32)  # noqa: E731
        values = lambda: t("values", (3, 4), I64)  # noqa: E731
        matrix = lambda: t("matrix", (4, L, N), dt)  # noqa: E731
        c("quantize_rows", lambda: pnns.quantize_rows(vectors(), 2.5, stream))
        c("diagonal_matrix", lambda: pnns.diagonal_matrix(values(), stream=stream))
        c("diagonal_matrix given", lambda: pnns.diagonal_matrix(values(), 2, True, 1, stream))
        c("process_database", lambda: pnns.process_database(vectors(), 2.5, stream=stream))
        key = lambda label: t(label, (L, 2, L + 1, N), dt)  # noqa: E731
        pairs = lambda: [(key("minus1"), None), (key("minus1'"), key("minusBaby'"))]  # noqa: E731
        for method in ("mul_transpose", "compute_response"):
            c(method, lambda: getattr(pnns, method)(matrix(), 3, 4, t("queries", (2, 2, L, N), dt), None, stream=stream))
            c(f"{method} keys", lambda: getattr(pnns, method)(matrix(), 3, 4, t("queries", (2, 2, L, N), dt), pairs(), 2, stream))
        plan = [(1, 2), (-3, 1)]
        rows = lambda: [[key(f"key{q}{k}") if (q + k) % 3 else None for k in range(4 + len(plan))] for q in range(2)]  # noqa: E731
        for method in ("mul_transpose_matrix", "compute_response_matrix"):
            c(method, lambda: getattr(pnns, method)(matrix(), 3, 4, t("queries", (2, 2, 2, L, N), dt), 5, None, None,
                                                    stream=stream))
            c(f"{method} keys", lambda: getattr(pnns, method)(matrix(), 3, 4, t("queries", (2, 2, 2, L, N), dt), 5, plan, rows(),
                                                              2, stream))

    # ---- SimplePirServer / SimplePirServer32
    for name, dt in (("SimplePirServer", I64), ("SimplePirServer32", I32)):
        cls = getattr(heamd, name)
        entries = lambda: t("entries", (4, 5), U8)  # noqa: E731
        seed = lambda: t("seed", (32,), U8)  # noqa: E731
        c = lambda method, call, n=name: case(f"{n}.{method}", call)  # noqa: E731
        server = c("process", lambda: cls.process(entries(), 8, 32, 16, seed(), stream))
        params = dict(server.params)
        c("reprocess", lambda: server.reprocess(entries(), seed(), stream))
        c("reprocess seed bytes", lambda: server.reprocess(entries(), bytes(range(32)), stream))
        c("reprocess out", lambda: server.reprocess(entries(), seed(), stream, (t("database", (6, 4), U8), t("hint", (6, 16), dt))))
        c("wide_database", lambda: server.wide_database(stream))
        c("compute_response", lambda: server.compute_response(t("requests", (2, 4), dt), stream))
        c("compute_response_batch", lambda: server.compute_response_batch(t("requests", (2, 4), dt), stream))
        c("from_wide", lambda: cls.from_wide(t("wide", (6, 4), dt), t("hint", (6, 16), dt), params, stream).database)
    return table


def record(monkeypatch):
    import heamd

    with recording(monkeypatch) as rec:
        return json.loads(json.dumps(drive(heamd, rec)))


def test_call_shapes(monkeypatch):
    with open(TABLE) as f:
        expected = json.load(f)
    got = record(monkeypatch)
    assert sorted(got) == sorted(expected)
    for name in expected:
        assert got[name] == expected[name], name


# The `_u32` rows of SIGNATURES as they stood while each was spelled out beside its 8-byte twin: v void*, z size_t / uint64_t,
# w uint32_t, i int, Px a pointer to x.
TWIN_ARGTYPES = {
    "he_ntt_forward_device_u32": "v v z v",
    "he_ntt_inverse_device_u32": "v v z v",
    "he_poly_add_device_u32": "v v v z v",
    "he_poly_sub_device_u32": "v v v z v",
    "he_poly_neg_device_u32": "v v z v",
    "he_poly_mul_device_u32": "v v v z v",
    "he_poly_mul_scalar_device_u32": "v v Pw z v",
    "he_poly_divide_and_round_q_last_device_u32": "v v v z v",
    "he_poly_serialize_device_u32": "v v z i v v",
    "he_poly_deserialize_device_u32": "v v z z i v v",
    "he_poly_random_from_seeds_device_u32": "v v z v v",
    "he_ciphertexts_serialize_device_u32": "v v z w Pi v z v",
    "he_ciphertexts_deserialize_device_u32": "v v z z w Pi v v v",
    "he_ciphertexts_deserialize_seeded_device_u32": "v v z v z i v v",
    "he_bfv_context_create_u32": "w z Pz w Pv",
    "he_rns_lift_q_to_qbsk_device_u32": "v w v v z v",
    "he_rns_floor_qbsk_to_q_device_u32": "v w v v z v",
    "he_rns_scale_and_round_device_u32": "v w v z v z v",
    "he_bfv_mul_device_u32": "v w v v v z v z v",
    "he_bfv_relinearize_device_u32": "v w v v v z v z v",
    "he_bfv_apply_galois_device_u32": "v w v z v v z v z v",
    "he_bfv_mod_switch_down_device_u32": "v w w v v z v",
    "he_bfv_mul_plain_device_u32": "v w w v v z v",
    "he_bfv_add_plain_device_u32": "v w w v v z v",
    "he_bfv_sub_plain_device_u32": "v w w v v z v",
    "he_bfv_inner_product_plain_resident_device_u32": "v w w v v v z z v v",
    "he_bfv_inner_product_device_u32": "v w v v z v v z v",
    "he_bfv_inner_product_shared_device_u32": "v w v v z z v v",
    "he_pir_compute_response_device_u32": "v Pw w v v z v v z v v v",
    "he_pir_compute_response_queries_device_u32": "v Pw w z v v z v v z Pv v v",
    "he_pir_compute_response_to_query_device_u32": "v Pw w v z z Pz Pv z v Pv Pv z z v v",
    "he_bfv_plaintext_to_eval_device_u32": "v w v v z v",
    "he_bfv_plaintext_to_coeff_device_u32": "v w v v z v",
    "he_pir_process_database_device_u32": "v Pw w v Pz z z i v v v",
    "he_pir_database_load_device_u32": "v v z v z v v v",
    "he_pir_database_save_device_u32": "v v v z v z v v",
    "he_simple_pir_process_database_device_u32": "v v v v v v",
    "he_simple_pir_pack_database_device_u32": "w v v z v",
    "he_simple_pir_unpack_database_device_u32": "w v v z v",
    "he_simple_pir_compute_response_device_u32": "w w v z z v z v v",
    "he_simple_pir_compute_response_batch_device_u32": "w w v z z v z v v",
    "he_pnns_context_create_u32": "v Pv",
    "he_pnns_diagonal_matrix_device_u32": "v v z z w i w v v v",
    "he_pnns_mul_transpose_device_u32": "v v z z z w v z v v v",
    "he_pnns_compute_response_device_u32": "v v z z z w v z v v v",
    "he_pnns_mul_transpose_matrix_device_u32": "v v z z z w v z z v z v v v",
    "he_pnns_compute_response_matrix_device_u32": "v v z z z w v z z v z v v v",
}
_CODES = {"v": ctypes.c_void_p, "z": ctypes.c_size_t, "w": ctypes.c_uint32, "i": ctypes.c_int}


def _argtypes(text):
    return [ctypes.POINTER(_CODES[code[1]]) if code[0] == "P" else _CODES[code] for code in text.split()]


def test_u32_signatures_are_those_spelled_out_before():
    import heamd

    assert ctypes.c_size_t is ctypes.c_uint64  # (the snapshot does not tell them apart)
    rows = {name: (restype, argtypes) for name, restype, argtypes in heamd.binding.SIGNATURES}
    assert len(rows) == len(heamd.binding.SIGNATURES)
    assert {name for name in rows if name.endswith("_u32")} == set(TWIN_ARGTYPES)
    for name, text in TWIN_ARGTYPES.items():
        assert rows[name] == (ctypes.c_int, _argtypes(text)), name


if __name__ == "__main__":
    import sys

    import pytest

    sys.path.append(os.path.join(os.path.dirname(TABLE), "..", "swift-homomorphic-encryption_amd"))
    patch = pytest.MonkeyPatch()
    with open(TABLE, "w") as f:
        json.dump(record(patch), f, indent=0, sort_keys=True)
        f.write("\n")
    patch.undo()
