"""What the key-generation and encryption methods of BfvContext / BfvContext32 / PolyContext hand to C, without a device or a
built library (binding_recorder.py, as test_decrypt_call_shapes.py does for decryption): the entry, the arguments in order --
the slab word first among them, since these entries have no `_u32` twins -- and the dtype and shape of what comes back, N = 8,
L = 2 (three coefficient moduli), batch 3."""
import torch

import binding_recorder
from binding_recorder import BATCH, DEGREE, MODULI, Stream, recording

N, L, B = DEGREE, MODULI, BATCH
U8 = torch.uint8


def _drive(monkeypatch, cls_name, dtype, word_bits):
    import heamd

    monkeypatch.setitem(binding_recorder.RETURNS, "he_bfv_encrypt_workspace_bytes", 4096)
    with recording(monkeypatch) as rec:
        stream = Stream()
        bfv = getattr(heamd, cls_name)(N, 17, [97, 193, 257])
        name = str(dtype)

        def run(call, host_len=0):
            rec.calls.clear()
            rec.made, rec.host_len = 0, host_len
            value = call()
            return [list(c) for c in rec.calls], rec.result(value)

        key = lambda: rec.tensor("key", (L + 1, N), dtype)  # noqa: E731
        seeds = lambda label, *shape: rec.tensor(label, shape + (32,), U8)  # noqa: E731
        workspace = lambda: rec.tensor("workspace", (64,), U8)  # noqa: E731

        calls, result = run(lambda: bfv.generate_secret_key(seeds("seeds", B), stream))
        assert calls == [["he_bfv_generate_secret_key_device", [None, word_bits, "seeds", "new0", B, None, 0, "stream"]]]
        assert result == [name, [B, L + 1, N], "new0"]

        calls, result = run(lambda: bfv.encrypt_zero(key(), seeds("a", B), seeds("e", B), stream=stream))
        assert calls == [["he_bfv_encrypt_zero_device", [None, word_bits, L, 0, "key", "a", "e", "new0", B, None, 0, "stream"]]]
        assert result == [name, [B, 2, L, N], "new0"]
        calls, result = run(lambda: bfv.encrypt_zero(key(), seeds("a", B), seeds("e", B), L + 1, True, stream, workspace()))
        assert calls == [["he_bfv_encrypt_zero_device",
                          [None, word_bits, L + 1, 1, "key", "a", "e", "new0", B, "workspace", 64, "stream"]]]
        assert result == [name, [B, 2, L + 1, N], "new0"]

        calls, result = run(lambda: bfv.encrypt(rec.tensor("plaintexts", (B, N), dtype), key(), seeds("a", B), seeds("e", B), 1,
                                                stream, workspace()))
        assert calls == [["he_bfv_encrypt_device",
                          [None, word_bits, 1, "key", "a", "e", "plaintexts", "new0", B, "workspace", 64, "stream"]]]
        assert result == [name, [B, 2, 1, N], "new0"]

        calls, result = run(lambda: bfv.generate_key_switch_keys(key(), rec.tensor("current", (B, L + 1, N), dtype),
                                                                 seeds("a", B, L), seeds("e", B, L), stream))
        assert calls == [["he_bfv_generate_key_switch_keys_device",
                          [None, word_bits, "key", "current", "a", "e", "new0", B, None, 0, "stream"]]]
        assert result == [name, [B, L, 2, L + 1, N], "new0"]

        calls, result = run(lambda: bfv.generate_relinearization_key(key(), seeds("a", L), seeds("e", L), stream, workspace()))
        assert calls == [["he_bfv_generate_relinearization_key_device",
                          [None, word_bits, "key", "a", "e", "new0", "workspace", 64, "stream"]]]
        assert result == [name, [L, 2, L + 1, N], "new0"]

        calls, result = run(lambda: bfv.generate_galois_keys(key(), [3, 15], seeds("a", 2, L), seeds("e", 2, L), stream), host_len=2)
        assert calls == [["he_bfv_generate_galois_keys_device",
                          [None, word_bits, "key", [3, 15], 2, "a", "e", "new0", None, 0, "stream"]]]
        assert result == [name, [2, L, 2, L + 1, N], "new0"]

        calls, result = run(lambda: bfv.encrypt_workspace_bytes("galois_keys", 5))
        assert calls == [["he_bfv_encrypt_workspace_bytes", [None, word_bits, 5, L, 0, 5]]] and result == 4096
        calls, result = run(lambda: bfv.encrypt_workspace_bytes("encrypt_zero", B, L + 1, True))
        assert calls == [["he_bfv_encrypt_workspace_bytes", [None, word_bits, 1, L + 1, 1, B]]]

        # the polynomial-level samplers take the word as an argument of the method
        poly = heamd.PolyContext(N, [97, 193])
        for method, entry in ((poly.random_ternary_from_seeds, "he_poly_random_ternary_from_seeds_device"),
                              (poly.random_centered_binomial_from_seeds, "he_poly_random_centered_binomial_from_seeds_device")):
            word = heamd.binding.WORD32 if word_bits == 32 else heamd.binding.WORD64
            calls, result = run(lambda: method(seeds("seeds", B), word, stream))
            assert calls == [[entry, [None, word_bits, "seeds", B, "new0", "stream"]]]
            assert result == [name, [B, MODULI, N], "new0"]


def test_encrypt_call_shapes_8_byte_words(monkeypatch):
    _drive(monkeypatch, "BfvContext", torch.int64, 64)


def test_encrypt_call_shapes_4_byte_words(monkeypatch):
    _drive(monkeypatch, "BfvContext32", torch.int32, 32)
