"""Every `*_device` entry of tests/aliasing_cases.py held to its memory footprint, on a device, under poisoned scratch.

The suite's other files check the words a call returns; this one checks the bytes it touches.  Each row x slab word x shape of
tests/footprint_cases.py runs on one arena of tests/footprint.py: the call's slabs between guard bytes, every slab exactly its
stated bytes, the workspace exactly the bytes its `*_workspace_bytes` function reports.  Pure outputs and the workspace are
poisoned, once with 0xA5 bytes and once with 0xFF bytes (words above every modulus), and after each call

  * the status is HE_OK;
  * outside the slabs the row writes the arena reads as it was filled: the guards, the padding, every read-only slab bit for
    bit, and the bytes behind workspace + workspace_bytes;
  * the outputs of the two poison runs are byte-identical -- a form that reads scratch it did not write, or leaves a word of
    its output unwritten, cannot give the same bytes over 0xA5.. and 0xFF..;
  * with a workspace: the outputs equal those of the call with workspace = NULL (during which the workspace slab is one more
    slab the call must leave alone), and the call with the workspace 16 bytes short is HE_ERR_INVALID_ARGUMENT and changes
    not one byte of the arena;
  * the six workspace pipelines and the decrypt dot product equal the CPU oracle word for word, at every shape -- the oracle
    calls of test_gpu_bfv.py, test_gpu_galois.py and test_gpu_decrypt.py.  The other rows' parity at these shapes is held by
    test_gpu_aliasing.py and test_gpu_grid_stride.py.

Which kernel form a shape takes cannot be observed through the library: the shapes of footprint_cases.FORMS follow from the
launchers' conditions as read, each cited next to its shape.  Every call here is a form the contract accepts, on memory the
test owns; reads past the end of an input are out of reach (they cannot be seen without a fault), but the padding next to every
input differs from run to run only where the poison does, so a stray read that changes the result fails the parity above.

The composite servers (PIR expansion and response, the two PNNS responses, the two SimplePIR responses; DEFERRED in the aliasing
table, and they stay so) run once each through the same arena, at the bottom of this file: every device input unchanged, the
Galois keys behind a host array of pointers included, `out` poisoned both ways, the words their own tests' reference gives.
Their scratch is the library's own stream-ordered memory and cannot be guarded.
"""
import ctypes

import numpy as np
import pytest

import aliasing_cases as A
import footprint
import footprint_cases as F
import heamd

pytestmark = pytest.mark.gpu

OK, INVALID = 0, 16
CASES = [(row, w, shp) for row in A.CASES for shp in F.shapes(row) for w in F.words_of(row, shp)]
IDS = ["%s-u%d-%s" % (row.name, 8 * w, shp.name) for row, w, shp in CASES]

_contexts = {}


def contexts(oracle, kind, word_bytes, degree, bits):
    """(ours, oracle's or None, the ring's coefficient moduli) of a ring, made once per module"""
    key = (kind, word_bytes, degree, bits)
    if key not in _contexts:
        word_bits = 8 * word_bytes
        moduli = oracle.generate_primes(list(bits), False, degree, word_bits=word_bits)
        if kind == "bfv":
            t = oracle.generate_primes([A.PLAINTEXT_BITS], True, degree, word_bits=word_bits)[0]
            ours = (heamd.BfvContext32 if word_bytes == 4 else heamd.BfvContext)(degree, t, moduli)
            ref = oracle.BfvContext(degree, t, moduli, word_bits=word_bits)
        else:
            ours, ref = (heamd.PolyContext(degree, moduli) if kind == "poly" else None), None
        _contexts[key] = (ours, ref, [int(m) for m in moduli])
    return _contexts[key]


def residues(rng, nbytes, moduli, degree, word_bytes):
    """[items][len(moduli)][N], row r uniform below moduli[r]; the first item 0 and the last q - 1 (a slab of one or two items:
    its first and its last coefficient)"""
    per = len(moduli) * degree * word_bytes
    items = nbytes // per
    assert items * per == nbytes and items > 0, (nbytes, per)
    slab = np.stack([rng.integers(0, m, size=(items, degree), dtype=np.uint64) for m in moduli], axis=1)
    top = np.array(moduli, dtype=np.uint64) - np.uint64(1)
    if items >= 3:
        slab[0], slab[-1] = 0, top[:, None]
    else:
        slab[0, :, 0], slab[-1, :, -1] = 0, top
    return slab


def host_fill(kind, rng, nbytes, env, moduli, qbsk, t):
    """A slab's input as an array of its words (uint64 for residues whatever the slab word: the oracle's type)"""
    w, n = env["w"], env["N"]
    if kind in ("q", "all", "qbsk"):
        return residues(rng, nbytes, F.fill_rows(kind, env, moduli, qbsk), n, w)
    if kind == "t":
        values = rng.integers(0, t, size=(nbytes // (n * w), n), dtype=np.uint64)
        values[0], values[-1] = 0, t - 1
        return values
    if kind in ("seeds", "bytes"):
        return rng.integers(0, 256, size=nbytes, dtype=np.uint8)
    if kind == "words32":
        return rng.integers(0, 1 << 30, size=nbytes // 8, dtype=np.uint64)
    if kind == "flags":
        return rng.integers(0, 2, size=nbytes, dtype=np.uint8)
    if kind == "acc":
        pairs = rng.integers(0, 1 << 63, size=(nbytes // 16, 2), dtype=np.uint64)
        pairs[:, 1] >>= np.uint64(43)
        return pairs
    if kind in ("zero", "packed"):
        return np.zeros(nbytes, dtype=np.uint8)
    raise AssertionError(kind)


def as_bytes(array, kind, word_bytes):
    if kind in ("q", "all", "qbsk", "t") and word_bytes == 4:
        array = array.astype(np.uint32)
    return np.ascontiguousarray(array).reshape(-1).view(np.uint8)


def oracle_outputs(row, ref, env, host):
    """{slab: words} the CPU oracle gives for a row of F.ORACLE_ROWS -- the calls of test_gpu_bfv.py (mul, relinearize,
    innerProduct), test_gpu_galois.py (applyGalois) and test_gpu_decrypt.py (Case.oracle_dot)"""
    from conftest import host_threads

    L, n = env["L"], env["N"]
    if row.name == "he_bfv_mul_device":
        return {"out": ref.mul(host["lhs"], host["rhs"], L, threads=host_threads())}
    if row.name == "he_bfv_relinearize_device":
        return {"out": ref.relinearize(host["ct3"], host["key"], L, threads=host_threads())}
    if row.name == "he_bfv_apply_galois_device":
        return {"out": ref.apply_galois(host["ct"], env["element"], host["galois_key"], L)}
    if row.name == "he_bfv_apply_galois_grouped_device":
        groups = host["ct"].reshape(2, -1)
        return {"out": np.stack([ref.apply_galois(groups[g], env["element"], host["galois_keys[%d]" % g], L) for g in (0, 1)])}
    if row.name == "he_bfv_inner_product_device":
        return {"out": ref.inner_product(host["lhs"], host["rhs"], L)}
    assert row.name == "he_bfv_secret_dot_product_device"
    qctx, polys = ref.ciphertext_context(L), env["polys"]
    s, out = host["secret_key"].reshape(L, n), []
    for ct in host["cts"].reshape(env["batch"], polys, L, n):
        ct_eval = ct if env["is_eval"] else qctx.forward_ntt(ct)
        dot, power = ct_eval[0].copy(), s.copy()
        for index in range(1, polys):
            dot = qctx.add(dot, qctx.mul(ct_eval[index], power))
            power = qctx.mul(power, s)
        out.append(qctx.inverse_ntt(dot))
    return {"out": np.stack(out)}


@pytest.mark.parametrize("row,word_bytes,shp", CASES, ids=IDS)
def test_entry_keeps_to_its_footprint(oracle, monkeypatch, row, word_bytes, shp):
    import torch

    lib = heamd.load_library()
    degree = F.degree_of(row, shp)
    ours, ref, moduli = contexts(oracle, row.context, word_bytes, degree, shp.bits[8 * word_bytes])
    handle = ours.h if ours is not None else None
    name = row.name + "_u32" if (row.words == "twin" and word_bytes == 4) else row.name
    for variable, value in shp.setenv.items():
        monkeypatch.setenv(variable, value)
    env = F.environment(row, shp, moduli, word_bytes)
    sized = F.workspace_arguments(row, env)
    if sized is not None:
        function = getattr(lib, sized[0])
        function.restype = ctypes.c_size_t
        reported = int(function(handle, *sized[1]))
        # (the `_u32` twins: half the bytes the function reports, he_amd.h)
        env["workspace_bytes"] = reported // 2 if (row.words == "twin" and word_bytes == 4) else reported
        assert env["workspace_bytes"] >= 32, (sized, reported)
    sizes = A.slab_bytes(row, env)
    arena = footprint.layout(sizes, row.written)
    kinds = F.FILLS[row.name]
    spans = {slab: footprint.span(arena, slab) for slab in row.slabs}  # where the call sees each slab
    if shp.alias is not None:
        # the written slab at the read one's address, a form the row's `same` allows: the call updates the head of the read slab,
        # and the arena's own slab of that name is one more range it must leave as it was filled
        written_alias, read_alias = shp.alias
        assert A.may_be_same(row, written_alias, read_alias, env) and sizes[written_alias] <= sizes[read_alias]
        spans[written_alias] = (arena.offsets[read_alias], arena.offsets[read_alias] + sizes[written_alias])
    masked = [spans[slab] for slab in row.written]

    rng = np.random.default_rng(len(IDS) + sum(map(ord, name + shp.name)))
    qbsk = ours.qbsk_context(env["L"]).moduli if "qbsk" in kinds.values() else None
    t = ours.t if row.context == "bfv" else None
    host = {slab: host_fill(kind, rng, sizes[slab], env, moduli, qbsk, t) for slab, kind in kinds.items()
            if kind not in F.POISONED}
    device = {slab: torch.from_numpy(as_bytes(array, kinds[slab], word_bytes).copy()).cuda() for slab, array in host.items()}

    backing = torch.empty(arena.total + footprint.ALIGN, dtype=torch.uint8, device="cuda")
    skew = -backing.data_ptr() % footprint.ALIGN
    memory = backing[skew: skew + arena.total]
    where = {slab: memory.data_ptr() + begin for slab, (begin, _) in spans.items()}
    results = [slab for slab in row.written if slab != "workspace"]

    def fill(poison):
        memory.fill_(footprint.GUARD_BYTE)
        for slab, kind in kinds.items():
            begin, end = footprint.span(arena, slab)
            if kind in F.POISONED:
                memory[begin:end] = poison
            else:
                memory[begin:end] = device[slab]
        return memory.clone()

    def call(at=where, **changed):
        status, text = A.invoke(lib, row, name, handle, dict(env, **changed), at)
        torch.cuda.synchronize()
        return status, text

    outputs = []
    for poison in footprint.POISONS:
        filled = fill(poison)
        image, written = footprint.expected_image(arena, filled)
        assert shp.alias is not None or written == masked
        status, text = call()
        assert status == OK, (name, shp.name, hex(poison), status, text)
        footprint.verify(arena, memory, image, masked, "%s %s over 0x%02X" % (name, shp.name, poison))
        outputs.append({slab: memory[slice(*spans[slab])].clone() for slab in results})
    for slab in results:
        assert torch.equal(outputs[0][slab], outputs[1][slab]), "%s %s: %s depends on what its outputs and workspace held" % (
            name, shp.name, slab)

    if sized is not None:
        # workspace = NULL: the library's own scratch; the workspace slab is then one more slab to leave alone
        filled = fill(footprint.POISONS[0])
        status, text = call(at=dict(where, workspace=None), workspace_bytes=0)
        assert status == OK, (name, shp.name, "workspace = NULL", status, text)
        footprint.verify(arena, memory, filled, [spans[slab] for slab in results],
                         "%s %s with workspace = NULL" % (name, shp.name))
        for slab in results:
            assert torch.equal(memory[slice(*spans[slab])], outputs[0][slab]), (name, shp.name, slab, "workspace = NULL")
        # 16 bytes short: refused, nothing launched
        filled = fill(footprint.POISONS[0])
        status, text = call(workspace_bytes=env["workspace_bytes"] - 16)
        assert status == INVALID, (name, shp.name, "workspace 16 bytes short", status, text)
        footprint.verify(arena, memory, filled, [], "%s %s with the workspace 16 bytes short" % (name, shp.name))

    if row.name in F.ORACLE_ROWS:
        word = np.uint32 if word_bytes == 4 else np.uint64
        for slab, expected in oracle_outputs(row, ref, env, host).items():
            got = outputs[0][slab].cpu().numpy().view(word).astype(np.uint64)
            assert np.array_equal(got, np.asarray(expected).reshape(-1)), (name, shp.name, slab)


# ---- the composite servers: footprint only ----------------------------------------------------------------------------------
# The protocol entries stay DEFERRED in tests/aliasing_cases.py (what may alias among their arguments is not stated yet).  Here
# each runs once through the same arena: every device input -- the Galois keys reached through a host array of pointers
# included -- between guard bytes and unchanged after the call, `out` poisoned both ways, the words those of the reference its
# own test file compares with.  Their scratch is the library's own (stream-ordered, he_amd.h) and cannot be guarded.  The
# calls go through the binding, whose one allocation per call (heamd.binding._empty, the result) is handed the arena's `out`.
def through_the_arena(monkeypatch, inputs, out_shape, call, what):
    """inputs: {name: device tensor} in argument order; call(views) -> the result tensor of a binding method run on the arena's
    views of the inputs -> the result's words as a host array, after the checks above"""
    import collections

    import torch

    out_words = int(np.prod(out_shape))
    sizes = collections.OrderedDict((name, tensor.numel() * tensor.element_size()) for name, tensor in inputs.items())
    word_bytes = next(iter(inputs.values())).element_size()
    sizes["out"] = out_words * word_bytes
    arena = footprint.layout(sizes, ("out",))
    backing = torch.empty((arena.total + footprint.ALIGN) // 8 + 1, dtype=torch.int64, device="cuda").view(torch.uint8)
    skew = -backing.data_ptr() % footprint.ALIGN
    memory = backing[skew: skew + arena.total]
    views = {name: memory[slice(*footprint.span(arena, name))].view(tensor.dtype).view(tensor.shape)
             for name, tensor in inputs.items()}
    out_slab = memory[slice(*footprint.span(arena, "out"))]
    handed = []

    def hand_out(shape, word, device):
        assert not handed and int(np.prod(shape)) == out_words and word.bits == 8 * word_bytes, (what, shape, out_shape)
        handed.append(shape)
        return out_slab.view(getattr(torch, word.dtype)).view(tuple(shape))

    outputs = []
    with monkeypatch.context() as patch:
        patch.setattr(heamd.binding, "_empty", hand_out)
        for poison in footprint.POISONS:
            memory.fill_(footprint.GUARD_BYTE)
            for name, tensor in inputs.items():
                views[name].copy_(tensor)
            out_slab.fill_(poison)
            filled = memory.clone()
            image, masked = footprint.expected_image(arena, filled)
            del handed[:]
            got = call(views)
            torch.cuda.synchronize()
            assert handed and got.data_ptr() == out_slab.data_ptr(), what
            footprint.verify(arena, memory, image, masked, "%s over 0x%02X" % (what, poison))
            outputs.append(out_slab.clone())
    assert torch.equal(outputs[0], outputs[1]), "%s: out depends on what it held" % what
    return outputs[0].view(next(iter(inputs.values())).dtype).cpu().numpy()


def as_words(host, bits):
    word = np.uint32 if bits == 32 else np.uint64
    return host.view(word).astype(np.uint64)


@pytest.mark.parametrize("total", [1, 8])
def test_pir_expand_footprint(oracle, monkeypatch, total):
    """he_pir_expand_device at the ring of test_gpu_pir.py's `small` (N = 64), its smallest expansion (1: no level) and a full
    tree of three levels; uniform canonical words (word equality needs no valid encryption) against oracle.pir.expand"""
    import collections

    from test_gpu_pir import _uniform

    degree = 64
    t = oracle.generate_primes([17], True, degree)[0]
    q = oracle.generate_primes([40, 40, 40, 41], False, degree)
    ours, ref = heamd.BfvContext(degree, t, q), oracle.BfvContext(degree, t, q)
    rng = np.random.default_rng(total)
    query = _uniform(rng, (1, 2), q[:-1], degree)
    keys = {(degree >> k) + 1: _uniform(rng, (ours.L, 2), q, degree) for k in range(max((total - 1).bit_length(), 1))}
    inputs = collections.OrderedDict([("ciphertexts", heamd.to_device(query))])
    for element, key in keys.items():
        inputs["galois_keys[%d]" % element] = heamd.to_device(key)
    got = through_the_arena(monkeypatch, inputs, (total, 2, ours.L, degree),
                            lambda v: ours.pir_expand(v["ciphertexts"], total, {e: v["galois_keys[%d]" % e] for e in keys}),
                            "he_pir_expand_device")
    assert np.array_equal(as_words(got, 64), oracle.pir.expand(ref, query, total, keys).reshape(-1))


@pytest.mark.parametrize("bits", [64, 32])
def test_pir_compute_response_footprint(oracle, monkeypatch, bits):
    """he_pir_compute_response_device(_u32): dims [4, 3], three chunks, nil plaintexts in the second -- the shape of
    test_multi_chunk_response_matches_oracle at N = 64, and of test_pir_response_on_packed_uint32_slabs at its ring (N = 4096,
    27 / 28 / 28 bits) -- uniform words against the oracle's computeResponseForOneChunk per chunk"""
    import collections

    import torch

    from test_gpu_pir import _uniform

    if bits == 64:
        degree = 64
        t, q = oracle.generate_primes([17], True, degree)[0], oracle.generate_primes([40, 40, 40, 41], False, degree)
        ours, ref, dev = heamd.BfvContext(degree, t, q), oracle.BfvContext(degree, t, q), heamd.to_device
    else:
        degree, t, q = 4096, (1 << 16) + 1, [(1 << 27) - 40959, (1 << 28) - 65535, (1 << 28) - 73727]
        ours, ref, dev = heamd.BfvContext32(degree, t, q), oracle.BfvContext(degree, t, q, word_bits=32), heamd.to_device32
    rng = np.random.default_rng(bits)
    dims, chunks, per_chunk = [4, 3], 3, 12
    database = _uniform(rng, (chunks, per_chunk), q[:-1], degree)
    present = np.ones((chunks, per_chunk), dtype=np.uint8)
    present[1, [0, 7]] = 0
    dim0, rest = _uniform(rng, (dims[0], 2), q[:-1], degree), _uniform(rng, (dims[1], 2), q[:-1], degree)
    key = _uniform(rng, (ours.L, 2), q, degree)
    inputs = collections.OrderedDict([("dim0_query_eval", dev(dim0)), ("remaining_query", dev(rest)), ("database", dev(database)),
                                      ("present_device", torch.from_numpy(present).cuda()), ("relinearization_key", dev(key))])
    got = through_the_arena(monkeypatch, inputs, (chunks, 2, 1, degree), lambda v: ours.pir_compute_response(
        dims, v["dim0_query_eval"], v["remaining_query"], v["database"], chunks, present_device=v["present_device"],
        relinearization_key=v["relinearization_key"]), "he_pir_compute_response_device u%d" % bits)
    expected = [oracle.pir.compute_response_for_one_chunk(ref, dims, dim0, rest, database[c], present[c], key) for c in range(chunks)]
    assert np.array_equal(as_words(got, bits), np.stack(expected).reshape(-1))


@pytest.mark.parametrize("word32", [False, True])
def test_pnns_compute_response_footprint(oracle, monkeypatch, word32):
    """he_pnns_compute_response_device(_u32) at N = 64: 63 x 5 of test_gpu_pnns_response.py's grid, the smallest of its shapes
    that reads both Galois keys (baby_step 2, giant_step > 1), two queries; its reference: the mulTranspose(vector:)
    restatement over the oracle and the oracle's modSwitchDown chain"""
    import collections

    import pnns_reference as pnns
    from test_gpu_pnns_response import expected_words, get_setup, random_inputs, to_device

    s = get_setup(oracle, 64, word32=word32)
    rows, cols, queries = 63, 5, 2
    values, query, keys = random_inputs(s, np.random.default_rng(5), rows, cols, queries)
    baby_step, giant_step = pnns.baby_step_giant_step(cols)
    assert baby_step > 1 and giant_step > 1
    matrix, flag = s.pnns.diagonal_matrix(values, baby_step=baby_step)
    assert int(flag.item()) == 0
    inputs = collections.OrderedDict([("matrix", matrix), ("queries", to_device(s, query))])
    for client, pair in enumerate(keys):
        for slot, key in enumerate(pair):
            inputs["galois_keys[%d][%d]" % (client, slot)] = to_device(s, key)
    got = through_the_arena(monkeypatch, inputs, (queries, 1, 2, 1, s.degree), lambda v: s.pnns.compute_response(
        v["matrix"], rows, cols, v["queries"], [tuple(v["galois_keys[%d][%d]" % (c, k)] for k in (0, 1)) for c in range(queries)],
        baby_step=baby_step), "he_pnns_compute_response_device%s" % ("_u32" if word32 else ""))
    _, single = expected_words(s, s.to_host(matrix), rows, cols, baby_step, query, keys)
    assert np.array_equal(as_words(got, 32 if word32 else 64), single.reshape(-1))


@pytest.mark.parametrize("word32", [False, True])
def test_pnns_compute_response_matrix_footprint(oracle, monkeypatch, word32):
    """he_pnns_compute_response_matrix_device(_u32): the first row of test_gpu_pnns_matrix.TABLE (N = 64, L = 3, a 10 x 4
    matrix, query matrices of 3 rows, one client), its keys by element and its restatement"""
    import collections

    from test_gpu_pnns_matrix import Case, default_plan, setup_for
    from test_gpu_pnns_response import to_device

    degree, L, rows, cols, row_count, clients = 64, 3, 10, 4, 3, 1
    s = setup_for(oracle, degree, L, word32=word32)
    case = Case(s, rows, cols, row_count, clients, default_plan(degree, rows, cols, row_count), 11)
    inputs = collections.OrderedDict([("matrix", case.matrix), ("queries", to_device(s, case.query))])
    slots = case.device_keys()
    for client, row in enumerate(slots):
        for slot, key in enumerate(row):
            if key is not None:
                inputs["galois_keys[%d][%d]" % (client, slot)] = key  # (two slots of one element: two copies in the arena)
    _, single = case.expected()
    got = through_the_arena(monkeypatch, inputs, single.shape, lambda v: s.pnns.compute_response_matrix(
        v["matrix"], rows, cols, v["queries"], row_count, case.plan,
        [[v.get("galois_keys[%d][%d]" % (c, k)) for k in range(len(slots[c]))] for c in range(clients)],
        baby_step=case.baby_step), "he_pnns_compute_response_matrix_device%s" % ("_u32" if word32 else ""))
    assert np.array_equal(as_words(got, 32 if word32 else 64), single.reshape(-1))


@pytest.mark.parametrize("entry", ["compute_response", "compute_response_batch"])
@pytest.mark.parametrize("name", ["one-entry-u32", "one-entry-u64"])
def test_simple_pir_compute_response_footprint(monkeypatch, name, entry):
    """he_simple_pir_compute_response_device(_u32) and he_simple_pir_compute_response_batch_device(_u32) at the smallest shape
    of test_gpu_simple_pir.SHAPES (one entry of 50 bytes), three requests, against tests/simple_pir_reference.py"""
    import collections

    import simple_pir_reference as R
    from test_gpu_simple_pir import Case, _words_to_device

    case = Case(name)
    p, queries = case.params, 3
    requests = case.rng.integers(0, 1 << p["ciphertext_bits"], size=(queries, p["database_columns"]), dtype=np.uint64)
    requests[-1] = (1 << p["ciphertext_bits"]) - 1
    inputs = collections.OrderedDict([("requests", _words_to_device(requests, case.word_bits)), ("database", case.server.database)])
    server = type(case.server)(None, None, p)

    def call(views):
        server.database = views["database"]
        return getattr(server, entry)(views["requests"])

    got = through_the_arena(monkeypatch, inputs, (queries, p["column_size"]), call, "he_simple_pir_%s_device u%d" % (entry, case.word_bits))
    expected = R.compute_response(p, case.database, requests, case.word_bits).astype(np.uint64)
    assert np.array_equal(as_words(got, case.word_bits), expected.reshape(-1))
