"""The SimplePIR client on the device against tests/simple_pir_client_reference.py, word for word and byte for
byte: the cached a-polynomials, encryptZero at both standard deviations and in forced row blocks, the hint product at its
worst-case words and pass boundaries, precompute against its two halves and the reference, add(index:), the decryption of
responses, the whole loop process -> precompute -> add_indices -> compute_response -> decrypt_responses, the memory footprint of
the entries that take a workspace, and stream-ordered use.  Shapes: tests/simple_pir_client_cases.py."""
import collections
import ctypes

import numpy as np
import pytest

import encrypt_reference as E
import footprint
import simple_pir_client_cases as cases
import simple_pir_client_reference as C
import simple_pir_reference as R

pytestmark = pytest.mark.gpu

OK, INVALID = 0, 16
vp = ctypes.c_void_p


def to_device(values, word_bits):
    import heamd

    values = np.ascontiguousarray(values, dtype=np.uint64)
    return heamd.to_device(values) if word_bits == 64 else heamd.to_device32(values)


def to_host(tensor, word_bits):
    import heamd

    return heamd.to_host(tensor) if word_bits == 64 else heamd.to_host32(tensor)


def device_bytes(array):
    import torch

    return torch.from_numpy(np.ascontiguousarray(array, dtype=np.uint8)).cuda()


def device_indices(indices):
    import torch

    return torch.tensor(list(indices), dtype=torch.int64, device="cuda")


BATCH = 3


class Case:
    """A shape with its inputs, the numpy server's hint and the reference's secrets and un-noised samples, built once."""

    def __init__(self, name):
        import heamd
        import oracle

        self.name, self.word_bits = name, cases.SHAPES[name][5]
        self.params = p = cases.params_of(oracle, name)
        self.entries, self.seed, self.secret_seeds, self.error_seeds = cases.inputs_of(name, p, BATCH)
        self.stream = E.oracle_stream(oracle)
        self.polys = R.a_polynomials(oracle, p, self.seed)
        self.database = R.process_database(oracle, self.entries, p)
        self.hint = R.hint(p, self.database, R.materialize_a(p, self.polys))
        self.secrets = [C.secret_polynomials(p, self.secret_seeds[b], self.stream) for b in range(BATCH)]
        self.samples = [C.noiseless_sample(p, self.polys, s) for s in self.secrets]
        self.client = heamd.SimplePirClient(p, to_device(self.hint, self.word_bits), self.seed, self.word_bits)
        self._queries = {}

    def use(self, std_dev):
        import heamd

        self.client.error_std_dev = heamd.binding.SIMPLE_PIR_ERROR_STD_DEVS[std_dev]
        return self.client

    def queries(self, std_dev):
        """the reference's encryptZero of every query of the batch: [BATCH][chunks][database_columns]"""
        if std_dev not in self._queries:
            self._queries[std_dev] = np.stack([
                C.encrypt_zero(self.params, self.polys, self.secrets[b], self.error_seeds[b], std_dev, self.stream, self.samples[b])
                for b in range(BATCH)])
        return self._queries[std_dev]

    def results(self):
        return np.stack([C.secret_times_matrix(s, self.hint, self.params["modulus"]) for s in self.secrets])

    def secret_words(self, batch=BATCH):
        return to_device(np.stack([C.secret_words(self.params, s) for s in self.secrets[:batch]]), self.word_bits)


_cases = {}


def case_of(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.fixture(params=cases.CLIENT_SHAPES)
def case(request):
    return case_of(request.param)


def test_shapes_cover_what_they_claim():
    import oracle

    plan = {name: cases.params_of(oracle, name) for name in cases.CLIENT_SHAPES}
    for name in ("three-polys-u32", "three-polys-u64"):
        assert plan[name]["a_poly_count"] >= 3 and plan[name]["database_columns"] % plan[name]["lattice_dimension"] != 0
    assert plan["ref-large-u32"]["chunks_per_entry"] == 5 and plan["ref-large-u64"]["chunks_per_entry"] == 4
    for name in ("ref-large-u32", "ref-large-u64"):
        assert plan[name]["entry_size_in_scalar"] % plan[name]["chunks_per_entry"] != 0  # a padded chunk
    assert plan["ref-small-u32"]["lattice_dimension"] == 1024 and plan["one-entry-u32"]["entry_count"] == 1
    assert plan["bytes8-u64"]["modulus"].bit_length() == 56
    assert plan["columns-equal-n-u32"]["database_columns"] == plan["columns-equal-n-u32"]["lattice_dimension"]


def test_a_polynomials(case):
    import oracle

    p = case.params
    ring = oracle.PolyContext(p["lattice_dimension"], [p["modulus"]])
    expected = ring.forward_ntt(np.ascontiguousarray(case.polys[:, None, :]))[:, 0, :]
    assert np.array_equal(to_host(case.client.a_polynomials(), case.word_bits), expected)


# ---- encryptZero -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("std_dev", cases.STD_DEVS)
def test_encrypt_zero(case, std_dev, monkeypatch):
    client, expected = case.use(std_dev), case.queries(std_dev)
    seeds = device_bytes(case.error_seeds)
    whole = to_host(client.encrypt_zero(case.secret_words(), seeds), case.word_bits)
    assert np.array_equal(whole, expected)
    one = to_host(client.encrypt_zero(case.secret_words(1), seeds[:1].contiguous()), case.word_bits)
    assert np.array_equal(one, expected[:1])
    if std_dev == "stdDev64" and case.name.startswith("ref-small"):
        plan = client.plan(BATCH)
        assert plan["error_stream_bytes"] == 32 and plan["query_words"] * plan["error_stream_bytes"] > 4 * 4096  # several refills
    unforced = client.plan(BATCH)["row_block"]
    for block in (1, 2):
        monkeypatch.setenv("HEAMD_SIMPLE_PIR_CLIENT_ROW_BLOCK", str(block))
        assert client.plan(BATCH)["row_block"] == block < unforced
        again = to_host(client.encrypt_zero(case.secret_words(), seeds), case.word_bits)
        assert np.array_equal(again, whole), block


# ---- secret x hint ---------------------------------------------------------------------------------------------------------------------
_rings = {}


def ring_client(n, cbits, word_bits):
    """a client whose context has the ring of (N, c): the hint of the product is an argument"""
    import heamd
    import oracle

    key = (n, cbits, word_bits)
    if key not in _rings:
        params = R.shape(oracle, 7, cbits, n, 4, 4, word_bits)
        assert params["modulus"].bit_length() == cbits + 1
        _rings[key] = heamd.SimplePirClient(params, to_device(np.zeros((1, n)), word_bits), bytes(32), word_bits)
    return _rings[key]


def check_product(client, secrets, hint):
    p = client.params["modulus"]
    got = to_host(client.secret_times_hint(to_device(C.secret_words(client.params, secrets), client.word_bits),
                                           hint=to_device(hint, client.word_bits)), client.word_bits)
    assert got.shape == (len(secrets), len(hint))
    assert np.array_equal(got, C.secret_times_matrix(secrets, hint, p))


@pytest.mark.parametrize("n", [64, 1024])
@pytest.mark.parametrize("cbits,word_bits", [(60, 64), (29, 32)])
def test_hint_product_worst_case_words(n, cbits, word_bits):
    """Every hint word p - 1: all +1 (terms p - 1), all -1 (terms 1) and alternating secrets, and a zero hint under -1 (terms p,
    the largest a lane adds).  At c = 60 a 64-bit word holds 8 to 15 such terms: the folds are what keeps the sums exact."""
    client = ring_client(n, cbits, word_bits)
    p = client.params["modulus"]
    assert client.plan()["fold_terms"] == ((1 << 64) - 1) // p and (cbits != 60 or client.plan()["fold_terms"] < 16)
    alternating = np.where(np.arange(n) % 2 == 0, 1, -1)
    secrets = np.stack([np.ones(n, dtype=np.int64), -np.ones(n, dtype=np.int64), alternating, -alternating])
    check_product(client, secrets, np.full((5, n), p - 1, dtype=np.uint64))
    check_product(client, secrets, np.zeros((5, n), dtype=np.uint64))


@pytest.mark.parametrize("cbits,word_bits", [(60, 64), (29, 32), (42, 64)])
def test_hint_product_passes_and_tiles(cbits, word_bits):
    """Random ternary rows at every pass boundary, over 130 hint rows: two full tiles of 64 and a partial one."""
    client = ring_client(64, cbits, word_bits)
    group = client.plan()["secret_rows_per_pass"]
    rng = np.random.default_rng(cbits)
    hint = rng.integers(0, client.params["modulus"], size=(130, 64), dtype=np.uint64)
    for rows in (1, group - 1, group, group + 1, 2 * group + 3):
        check_product(client, rng.integers(-1, 2, size=(rows, 64), dtype=np.int64), hint)


@pytest.mark.parametrize("n,cbits,word_bits", [(1024, 60, 64), (1024, 29, 32), (2048, 60, 64), (4096, 28, 32)])
def test_hint_product_long_rows(n, cbits, word_bits):
    """N = 1024 fills the code slab; above it the codes of a pass come slab by slab and the folds carry on across slabs."""
    client = ring_client(n, cbits, word_bits)
    rng = np.random.default_rng(n + cbits)
    hint = rng.integers(0, client.params["modulus"], size=(70, n), dtype=np.uint64)
    hint[0] = client.params["modulus"] - 1
    check_product(client, rng.integers(-1, 2, size=(client.plan()["secret_rows_per_pass"] + 1, n), dtype=np.int64), hint)


def test_hint_product_refuses_a_misaligned_hint():
    import heamd
    import torch

    client = ring_client(64, 60, 64)
    lib = heamd.load_library()
    secrets = to_device(np.zeros((1, 64)), 64)
    backing = torch.zeros(5 * 64 + 2, dtype=torch.int64, device="cuda")
    results = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    workspace = torch.zeros(client.workspace_bytes("secret_times_hint", 1), dtype=torch.uint8, device="cuda")
    assert backing.data_ptr() % 16 == 0

    def call(hint_address):
        status = lib.he_simple_pir_secret_times_hint_device(client.h, 64, vp(secrets.data_ptr()), 1, vp(hint_address), 5,
                                                            vp(results.data_ptr()), vp(workspace.data_ptr()), workspace.numel(), None)
        torch.cuda.synchronize()
        return status

    assert call(backing.data_ptr() + 8) == INVALID and b"16-byte" in lib.he_last_error_message()
    assert int((results == -1).sum()) == 5  # nothing launched
    assert call(backing.data_ptr()) == OK and int(results.count_nonzero()) == 0


# ---- precompute ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("std_dev", cases.STD_DEVS)
def test_precompute(case, std_dev):
    import torch

    client = case.use(std_dev)
    queries, results = client.precompute(device_bytes(case.secret_seeds), device_bytes(case.error_seeds))
    lower_queries = client.encrypt_zero(case.secret_words(), device_bytes(case.error_seeds))
    flat = case.secret_words().reshape(-1, case.params["lattice_dimension"])
    lower_results = client.secret_times_hint(flat).reshape(results.shape)
    assert torch.equal(queries, lower_queries) and torch.equal(results, lower_results)
    assert np.array_equal(to_host(queries, case.word_bits), case.queries(std_dev))
    assert np.array_equal(to_host(results, case.word_bits), case.results())


# ---- add(index:) and decrypt -----------------------------------------------------------------------------------------------------------
def test_add_indices(case):
    p = case.params
    count = p["entry_count"]
    indices = [0, count - 1, count // 2, count]  # first, last, middle, one past the end
    before = np.stack([case.queries("stdDev32")[b % BATCH] for b in range(4)])
    queries = to_device(before, case.word_bits)
    flags = case.client.add_indices(queries, device_indices(indices))
    assert flags.cpu().tolist() == [0, 0, 0, 1]
    after = to_host(queries, case.word_bits)
    for b in range(3):
        assert np.array_equal(after[b], C.add(p, before[b], indices[b])), b
        assert int((after[b] != before[b]).sum()) == p["chunks_per_entry"]  # one word per chunk, the rest untouched
    assert np.array_equal(after[3], before[3])
    # the word that wraps: 2^c - 1 + delta under the mask
    full = to_device(np.full_like(before[:1], (1 << p["ciphertext_bits"]) - 1), case.word_bits)
    case.client.add_indices(full, device_indices([count - 1]))
    assert np.array_equal(to_host(full, case.word_bits)[0], C.add(p, np.full_like(before[0], (1 << p["ciphertext_bits"]) - 1), count - 1))


def test_decrypt_responses(case):
    """Any words decrypt the same way on both sides: uniform responses and results, and a flagged row of zero bytes."""
    p = case.params
    count, shape = p["entry_count"], (4, p["chunks_per_entry"], p["column_size"])
    rng = cases.rng_of(case.name, "decrypt")
    responses = rng.integers(0, 1 << p["ciphertext_bits"], size=shape, dtype=np.uint64)
    results = rng.integers(0, p["modulus"], size=shape, dtype=np.uint64)
    indices = [0, count - 1, count // 2, count + 7]
    entries, flags = case.client.decrypt(to_device(responses, case.word_bits), to_device(results, case.word_bits),
                                         device_indices(indices))
    assert flags.cpu().tolist() == [0, 0, 0, 1]
    entries = entries.cpu().numpy()
    for b in range(3):
        assert bytes(entries[b]) == C.decrypt(p, responses[b], results[b], indices[b], case.word_bits), b
    assert not entries[3].any()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("std_dev", cases.STD_DEVS)
@pytest.mark.parametrize("name", cases.END_TO_END)
def test_end_to_end_on_the_device(name, std_dev):
    """process -> precompute -> add_indices -> compute_response -> decrypt_responses, nothing on the host but the seeds and the
    indices: the entries come back."""
    import heamd
    import oracle
    import torch

    entry_count, entry_size, pbits, cbits, n, word_bits = cases.SHAPES[name]
    params = cases.params_of(oracle, name)
    indices = cases.end_to_end_indices(name, params)
    entries, seed, secret_seeds, error_seeds = cases.inputs_of(name, params, len(indices), std_dev)
    server_class = heamd.SimplePirServer if word_bits == 64 else heamd.SimplePirServer32
    server = server_class.process(device_bytes(entries), pbits, cbits, n, seed)
    assert server.params == params
    client = heamd.SimplePirClient(server.params, server.hint, seed, word_bits, std_dev)
    queries, results = client.precompute(device_bytes(secret_seeds), device_bytes(error_seeds))
    where = device_indices(indices)
    assert not client.add_indices(queries, where).any()
    requests = queries.reshape(-1, params["database_columns"])
    responses = server.compute_response(requests).reshape(results.shape)
    got, flags = client.decrypt(responses, results, where)
    assert not flags.any()
    assert torch.equal(got.cpu(), torch.from_numpy(entries[indices]))


# ---- argument errors behind a context --------------------------------------------------------------------------------------------------
def test_argument_errors():
    import heamd
    import torch

    lib = heamd.load_library()
    case = case_of("ref-large-u32")
    other = ring_client(64, 42, 64)
    client, p = case.use("stdDev32"), case.params
    a = client.a_polynomials()
    torch.cuda.synchronize()
    secrets, seeds = case.secret_words(), device_bytes(case.error_seeds)
    queries = torch.full((BATCH, p["chunks_per_entry"], p["database_columns"]), -1, dtype=torch.int32, device="cuda")
    workspace = torch.zeros(client.workspace_bytes("encrypt_zero", BATCH), dtype=torch.uint8, device="cuda")

    def encrypt(ctx=client.h, bits=32, std_dev=0, batch=BATCH, ws=workspace.data_ptr(), ws_bytes=workspace.numel(), out=queries):
        status = lib.he_simple_pir_encrypt_zero_device(ctx, bits, std_dev, vp(a.data_ptr()), vp(secrets.data_ptr()),
                                                       vp(seeds.data_ptr()), vp(out.data_ptr()) if out is not None else None, batch,
                                                       vp(ws) if ws else None, ws_bytes, None)
        torch.cuda.synchronize()
        return heamd.binding.STATUS_NAMES[status]

    assert encrypt(bits=64) == "invalidArgument" and b"other word size" in lib.he_last_error_message()
    assert encrypt(ctx=other.h) == "invalidArgument"
    assert encrypt(bits=16) == "invalidArgument"
    assert encrypt(std_dev=2) == "invalidArgument" and b"standard deviation" in lib.he_last_error_message()
    assert encrypt(ws=0, ws_bytes=0) == "invalidArgument" and b"workspace" in lib.he_last_error_message()
    assert encrypt(ws_bytes=workspace.numel() - 16) == "invalidArgument"
    assert encrypt(ws=workspace.data_ptr() + 8, ws_bytes=workspace.numel() - 8) == "invalidArgument"
    assert encrypt(out=None) == "invalidArgument"
    assert encrypt(batch=(1 << 20) + 1) == "invalidArgument"
    assert int((queries == -1).sum()) == queries.numel()  # nothing was launched by any of them
    assert encrypt(batch=0) == "ok" and encrypt(batch=0, out=None, ws=0, ws_bytes=0) == "ok"
    assert encrypt(batch=0, std_dev=2) == "invalidArgument" and encrypt(batch=0, bits=64) == "invalidArgument"
    assert int((queries == -1).sum()) == queries.numel()
    assert encrypt() == "ok" and np.array_equal(to_host(queries, 32), case.queries("stdDev32"))
    assert int(workspace.count_nonzero()) == 0
    # batch 0 of the others
    none = vp()
    assert lib.he_simple_pir_precompute_queries_device(client.h, 32, 0, none, none, none, none, none, none, 0, none, 0, None) == OK
    assert lib.he_simple_pir_precompute_queries_device(client.h, 32, 2, none, none, none, none, none, none, 0, none, 0, None) == INVALID
    assert lib.he_simple_pir_secret_times_hint_device(client.h, 32, none, 0, none, 5, none, none, 0, None) == OK
    assert lib.he_simple_pir_add_indices_device(client.h, 32, none, none, none, 0, None) == OK
    assert lib.he_simple_pir_decrypt_responses_device(client.h, 32, none, none, none, none, none, 0, none, 0, None) == OK
    assert lib.he_simple_pir_add_indices_device(client.h, 64, none, none, none, 0, None) == INVALID
    assert lib.he_simple_pir_a_polynomials_device(client.h, 32, vp(client.seed.data_ptr()), vp(a.data_ptr()), none, 0, None) == INVALID
    for operation, count in (("a_polynomials", 1), ("encrypt_zero", BATCH), ("secret_times_hint", BATCH * 5), ("precompute", BATCH),
                             ("decrypt_responses", BATCH)):
        assert client.workspace_bytes(operation, count) == client.plan(BATCH)[operation + "_workspace_bytes"], operation


# ---- footprint -------------------------------------------------------------------------------------------------------------------------
def check_footprint(what, inputs, outputs, workspace_bytes, invoke):
    """One call on one arena (tests/footprint.py), the pattern of tests/test_gpu_pir_client.py: `inputs` {slab: uint8 device
    tensor} are only read, `outputs` {slab: bytes} are poisoned and written, then the workspace.  invoke(addresses,
    workspace_bytes) -> status.  -> {slab: bytes of the result}"""
    import heamd
    import torch

    assert workspace_bytes >= 32 and workspace_bytes % 16 == 0
    sizes = collections.OrderedDict((name, tensor.numel()) for name, tensor in inputs.items())
    sizes.update(outputs)
    sizes["workspace"] = workspace_bytes
    arena = footprint.layout(sizes, tuple(outputs) + ("workspace",))
    backing = torch.empty(arena.total + footprint.ALIGN, dtype=torch.uint8, device="cuda")
    skew = -backing.data_ptr() % footprint.ALIGN
    memory = backing[skew: skew + arena.total]
    spans = {name: footprint.span(arena, name) for name in sizes}
    where = {name: memory.data_ptr() + begin for name, (begin, _) in spans.items()}

    def fill(poison):
        memory.fill_(footprint.GUARD_BYTE)
        for name, tensor in inputs.items():
            memory[slice(*spans[name])] = tensor.reshape(-1)
        for name in list(outputs) + ["workspace"]:
            memory[slice(*spans[name])] = poison
        return memory.clone()

    def call(at, nbytes):
        status = invoke(at, nbytes)
        torch.cuda.synchronize()
        return status

    runs = []
    for poison in footprint.POISONS:
        image, masked = footprint.expected_image(arena, fill(poison))
        assert call(where, workspace_bytes) == OK, (what, hex(poison), heamd.load_library().he_last_error_message())
        footprint.verify(arena, memory, image, masked, "%s over 0x%02X" % (what, poison))
        # the secret- and error-dependent regions -- the whole workspace -- read zero once the stream has drained
        assert int(memory[slice(*spans["workspace"])].count_nonzero()) == 0, what
        runs.append({name: memory[slice(*spans[name])].clone() for name in outputs})
    for name in outputs:
        assert torch.equal(runs[0][name], runs[1][name]), "%s: %s depends on what its outputs and workspace held" % (what, name)
    # workspace = NULL, and 16 bytes short: refused, nothing launched
    for at, nbytes, how in ((dict(where, workspace=None), 0, "workspace = NULL"), (where, workspace_bytes - 16, "16 bytes short")):
        filled = fill(footprint.POISONS[0])
        assert call(at, nbytes) == INVALID, (what, how)
        footprint.verify(arena, memory, filled, [], "%s with %s" % (what, how))
    return {name: tensor for name, tensor in runs[0].items()}


def as_bytes(tensor):
    import torch

    return tensor.contiguous().view(torch.uint8).reshape(-1)


def at(addresses, name):
    return vp(addresses[name]) if addresses[name] is not None else None


@pytest.mark.parametrize("name,std_dev", [("ref-large-u32", "stdDev64"), ("three-polys-u64", "stdDev32")])
def test_footprint(name, std_dev):
    import heamd
    import torch

    lib, case = heamd.load_library(), case_of(name)
    client, p, bits = case.use(std_dev), case.params, case.word_bits
    word_bytes, code = bits // 8, client.error_std_dev
    a = client.a_polynomials()
    torch.cuda.synchronize()
    query_bytes = BATCH * p["chunks_per_entry"] * p["database_columns"] * word_bytes
    result_bytes = BATCH * p["chunks_per_entry"] * p["column_size"] * word_bytes
    # precompute
    inputs = collections.OrderedDict([("a", as_bytes(a)), ("hint", as_bytes(client.hint)),
                                      ("secret_seeds", device_bytes(case.secret_seeds).reshape(-1)),
                                      ("error_seeds", device_bytes(case.error_seeds).reshape(-1))])
    got = check_footprint("precompute", inputs, collections.OrderedDict([("queries", query_bytes), ("results", result_bytes)]),
                          client.workspace_bytes("precompute", BATCH),
                          lambda w, n: lib.he_simple_pir_precompute_queries_device(
                              client.h, bits, code, at(w, "a"), at(w, "hint"), at(w, "secret_seeds"), at(w, "error_seeds"),
                              at(w, "queries"), at(w, "results"), BATCH, at(w, "workspace"), n, None))
    word = np.uint64 if bits == 64 else np.uint32
    assert np.array_equal(got["queries"].cpu().numpy().view(word).reshape(case.queries(std_dev).shape), case.queries(std_dev))
    assert np.array_equal(got["results"].cpu().numpy().view(word).reshape(case.results().shape), case.results())
    # encrypt_zero
    inputs = collections.OrderedDict([("a", as_bytes(a)), ("secrets", as_bytes(case.secret_words())),
                                      ("error_seeds", device_bytes(case.error_seeds).reshape(-1))])
    again = check_footprint("encrypt_zero", inputs, collections.OrderedDict([("queries", query_bytes)]),
                            client.workspace_bytes("encrypt_zero", BATCH),
                            lambda w, n: lib.he_simple_pir_encrypt_zero_device(
                                client.h, bits, code, at(w, "a"), at(w, "secrets"), at(w, "error_seeds"), at(w, "queries"), BATCH,
                                at(w, "workspace"), n, None))
    assert torch.equal(again["queries"], got["queries"])
    # decrypt_responses
    rng = cases.rng_of(name, "footprint")
    shape = (BATCH, p["chunks_per_entry"], p["column_size"])
    responses = rng.integers(0, 1 << p["ciphertext_bits"], size=shape, dtype=np.uint64)
    indices = [0, p["entry_count"] - 1, p["entry_count"]]
    inputs = collections.OrderedDict([("responses", as_bytes(to_device(responses, bits))), ("results", got["results"]),
                                      ("indices", as_bytes(device_indices(indices)))])
    outputs = collections.OrderedDict([("entries", BATCH * p["entry_size_in_bytes"]), ("flags", BATCH * 4)])
    out = check_footprint("decrypt_responses", inputs, outputs, max(client.workspace_bytes("decrypt_responses", BATCH), 32),
                          lambda w, n: lib.he_simple_pir_decrypt_responses_device(
                              client.h, bits, at(w, "responses"), at(w, "results"), at(w, "indices"), at(w, "entries"), at(w, "flags"),
                              BATCH, at(w, "workspace"), n, None))
    entries = out["entries"].cpu().numpy().reshape(BATCH, -1)
    for b in range(2):
        assert bytes(entries[b]) == C.decrypt(p, responses[b], case.results()[b], indices[b], bits), b
    assert not entries[2].any() and out["flags"].cpu().numpy().view(np.uint32).tolist() == [0, 0, 1]


# ---- stream order ----------------------------------------------------------------------------------------------------------------------
def test_two_batches_back_to_back_on_one_stream():
    """No host synchronisation between two precompute calls and their uses on one stream; a workspace shared by both calls is the
    hazard: the second call may not start before the first one's zeroization, nor the first one's results be lost."""
    import torch

    case = case_of("ref-large-u64")
    client = case.use("stdDev32")
    first_seeds = (device_bytes(case.secret_seeds), device_bytes(case.error_seeds))
    second_seeds = (device_bytes(case.secret_seeds[::-1].copy()), device_bytes(case.error_seeds[::-1].copy()))
    alone = [client.precompute(*seeds) for seeds in (first_seeds, second_seeds)]
    torch.cuda.synchronize()
    workspace = torch.empty(client.workspace_bytes("precompute", BATCH), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        together = [client.precompute(*seeds, stream=stream, workspace=workspace) for seeds in (first_seeds, second_seeds)]
    stream.synchronize()
    for (queries, results), (expected_queries, expected_results) in zip(together, alone):
        assert torch.equal(queries, expected_queries) and torch.equal(results, expected_results)
    assert torch.equal(together[1][0], together[0][0].flip(0)) and int(workspace.count_nonzero()) == 0
    assert np.array_equal(to_host(together[0][0], 64), case.queries("stdDev32"))
