"""The wire entries at both ends of a MulPIR reply, at the smallest shape tests/test_gpu_pir.py uses: the
query and the evaluation key arrive as the bytes of `.seeded(poly0:seed:)`, he_ciphertexts_deserialize_seeded_device rebuilds
them on the device, he_pir_compute_response_to_query_device answers, and he_ciphertexts_serialize_device writes the reply
records with the skips of he_bfv_skip_lsbs_for_decryption -- equal, byte for byte, to the same chain composed from the oracle
and tests/ciphertext_wire_reference.py."""
import random

import numpy as np
import pytest

import ciphertext_wire_reference as R
import wire_format_reference as W
from bfv_helpers import BfvClient

pytestmark = pytest.mark.gpu


class SeededClient(BfvClient):
    """a client whose every uniform polynomial comes from a fresh 32-byte seed, as the reference's encryptor draws it when it
    is going to send `.seeded` (Bfv+Encrypt.swift:150-181); the seeds are kept in the order they were used"""

    def __init__(self, oracle, bfv_ctx, seed=0):
        super().__init__(oracle, bfv_ctx, seed)
        self.seeds = []

    def _uniform(self, poly_ctx):
        seed = bytes(self.rng.randrange(256) for _ in range(32))
        self.seeds.append(seed)
        return np.array(R.seeded_polynomial(seed, self.n, [int(q) for q in poly_ctx.moduli]), dtype=np.uint64)


def _compressed_query(ctx, total, ones):
    """PirUtil.compressInputsForOneCiphertext (PirUtil.swift:357-377)."""
    height = (total - 1).bit_length()
    inverse = pow(pow(2, height, ctx.t), -1, ctx.t)
    message = [0] * ctx.degree
    for index in ones:
        message[index] = inverse
    return message


def _seeded_in(poly_ctx, ciphertexts, seeds, coeff_format):
    """host ciphertexts [count][2][rows][N] whose slot 1 came from `seeds` -> the device tensor rebuilt from poly0 bytes + seeds"""
    import torch

    moduli = [int(q) for q in poly_ctx.moduli]
    widths = R.widths(moduli, 0)
    poly0 = b"".join(W.pack_record(ct[0].tolist(), widths) for ct in ciphertexts)
    assert len(poly0) == len(ciphertexts) * poly_ctx.serialization_byte_count(0)
    device_bytes = torch.from_numpy(np.frombuffer(poly0, dtype=np.uint8).copy()).cuda()
    device_seeds = torch.from_numpy(np.frombuffer(b"".join(seeds), dtype=np.uint8).copy()).cuda()
    return poly_ctx.ciphertexts_deserialize_seeded(device_bytes, device_seeds, len(ciphertexts), coeff_format)


def test_seeded_query_and_keys_in_reply_records_out(oracle):
    import heamd
    import torch

    degree = 64
    t = oracle.generate_primes([17], True, degree)[0]
    q = oracle.generate_primes([40, 40, 40, 41], False, degree)
    ref, ours = oracle.BfvContext(degree, t, q), heamd.BfvContext(degree, t, q)
    client = SeededClient(oracle, ref, seed=61)
    rng = random.Random(411)
    indices, dims, chunks, per_chunk = 1, [4, 3], 2, 12
    total = sum(dims) * indices
    entries = [[rng.randrange(ref.t) for _ in range(degree)] for _ in range(per_chunk * chunks)]
    database = ref.plaintext_to_eval(np.array(entries, dtype=np.uint64)).reshape(chunks, per_chunk, ref.L, degree)
    present = np.ones((chunks, per_chunk), dtype=np.uint8)
    a, b = 2, 1
    # ---- what the client sends: every ciphertext as poly0 bytes and a seed
    query = client.encrypt(_compressed_query(ref, total, [a, dims[0] + b]))[None]
    query_seeds, client.seeds = client.seeds, []
    elements = [(degree >> k) + 1 for k in range(max((total - 1).bit_length(), 1))]
    galois, galois_seeds = {}, {}
    for element in elements:
        galois[element] = client.galois_key(element)
        galois_seeds[element], client.seeds = client.seeds, []
    relin = client.relinearization_key()
    relin_seeds, client.seeds = client.seeds, []
    assert len(query_seeds) == 1 and all(len(s) == ref.L for s in list(galois_seeds.values()) + [relin_seeds])
    # ---- in: rebuilt on the device, word for word what the client holds
    ct_ctx, ks_ctx = ours.ciphertext_context(), ours.key_switching_context()
    device_query = _seeded_in(ct_ctx, query, query_seeds, coeff_format=1)
    assert np.array_equal(heamd.to_host(device_query), query)
    device_galois = {e: _seeded_in(ks_ctx, galois[e], galois_seeds[e], coeff_format=0) for e in elements}
    device_relin = _seeded_in(ks_ctx, relin, relin_seeds, coeff_format=0)
    for e in elements:
        assert np.array_equal(heamd.to_host(device_galois[e]), galois[e]), e
    assert np.array_equal(heamd.to_host(device_relin), relin)
    # ---- the reply
    got = ours.pir_compute_response_to_query(dims, device_query, indices, device_galois, device_relin,
                                             heamd.to_device(database), chunks,
                                             present_devices=torch.from_numpy(present).cuda())
    expanded = oracle.pir.expand(ref, query, total, galois)
    dim0 = np.stack([ref.ciphertext_context().forward_ntt(ct) for ct in expanded[: dims[0]]])
    expected = [oracle.pir.compute_response_for_one_chunk(ref, dims, dim0, expanded[dims[0]:], database[chunk], present[chunk],
                                                          relin) for chunk in range(chunks)]
    # ---- out: one call for every reply ciphertext, the skips of Bfv.skipLSBsForDecryption
    skips = heamd.skip_lsbs_for_decryption(degree, q[0], t, 1)
    assert skips == R.skip_lsbs_for_decryption(degree, q[0], t, 1) and skips[0] > skips[1] > 0
    reply_ctx = ours.ciphertext_context(1)
    records = reply_ctx.ciphertexts_serialize(got.reshape(indices * chunks, 2, 1, degree), skips).cpu().numpy()
    assert records.shape == (chunks, R.record_bytes(degree, [q[0]], skips))
    for chunk in range(chunks):
        want = R.pack_ciphertext(expected[chunk].tolist(), degree, [q[0]], skips)
        assert bytes(records[chunk]) == want, chunk
        # ... and what the client reads back decrypts to the entry
        _, polys = R.unpack_ciphertext(want, 2, degree, [q[0]], skips)
        assert client.decrypt(np.array(polys, dtype=np.uint64), moduli_count=1) == entries[chunk * per_chunk + a + dims[0] * b]
