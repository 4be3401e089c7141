"""What the decryption methods of BfvContext / BfvContext32 hand to C, without a device or a built library
(binding_recorder.py, as test_binding_call_shapes.py does for every other method): the entry, the arguments in order -- the
slab word first among them, since these entries have no `_u32` twins -- and the dtype and shape of what comes back, N = 8,
L = 2, batch 3."""
import torch

import binding_recorder
from binding_recorder import BATCH, DEGREE, MODULI, Stream, recording

N, L, B = DEGREE, MODULI, BATCH
LIMBS = 2


def _drive(monkeypatch, cls_name, dtype, word_bits, scheme_bits):
    import heamd

    monkeypatch.setitem(binding_recorder.RETURNS, "he_bfv_noise_norm_limbs", LIMBS)
    monkeypatch.setitem(binding_recorder.RETURNS, "he_bfv_decrypt_workspace_bytes", 4096)
    with recording(monkeypatch) as rec:
        stream = Stream()
        bfv = getattr(heamd, cls_name)(N, 17, [97, 193, 257], **({"word_bits": 32} if scheme_bits == 32 and cls_name == "BfvContext" else {}))
        name = str(dtype)

        def run(call):
            rec.calls.clear()
            rec.made, rec.host_len = 0, LIMBS
            value = call()
            return [list(c) for c in rec.calls], rec.result(value)

        cts = lambda polys=2: rec.tensor("cts", (B, polys, L, N), dtype)  # noqa: E731
        key = lambda: rec.tensor("key", (L + 1, N), dtype)  # noqa: E731
        workspace = lambda: rec.tensor("workspace", (64,), torch.uint8)  # noqa: E731

        calls, result = run(lambda: bfv.secret_dot_product(cts(), key(), stream=stream))
        assert calls == [["he_bfv_secret_dot_product_device",
                          [None, word_bits, L, 2, 0, "cts", "key", "new0", B, None, 0, "stream"]]]
        assert result == [name, [B, L, N], "new0"]
        calls, result = run(lambda: bfv.secret_dot_product(cts(3), key(), True, stream, workspace()))
        assert calls == [["he_bfv_secret_dot_product_device",
                          [None, word_bits, L, 3, 1, "cts", "key", "new0", B, "workspace", 64, "stream"]]]

        calls, result = run(lambda: bfv.decrypt(cts(), key(), stream=stream))
        assert calls == [["he_bfv_decrypt_device", [None, word_bits, L, 2, 0, "cts", "key", 1, "new0", B, None, 0, "stream"]]]
        assert result == [name, [B, N], "new0"]
        calls, result = run(lambda: bfv.decrypt(cts(1), key(), 5, True, stream, workspace()))
        assert calls == [["he_bfv_decrypt_device", [None, word_bits, L, 1, 1, "cts", "key", 5, "new0", B, "workspace", 64, "stream"]]]

        calls, result = run(lambda: bfv.noise_norm_device(cts(), key(), stream=stream))
        assert calls == [["he_bfv_noise_norm_limbs", [None, L]],
                         ["he_bfv_noise_norm_device", [None, word_bits, L, 2, 0, "cts", "key", "new0", B, None, 0, "stream"]]]
        assert result == ["torch.int64", [B, LIMBS], "new0"]  # limbs are 64-bit whatever the slab word
        calls, result = run(lambda: bfv.noise_norm(cts(3), key(), True, stream, workspace()))
        assert calls[1] == ["he_bfv_noise_norm_device",
                            [None, word_bits, L, 3, 1, "cts", "key", "new0", B, "workspace", 64, "stream"]]
        assert result == [0] * B  # Python integers

        calls, result = run(lambda: bfv.noise_budget(cts(), key(), stream=stream))
        assert [c[0] for c in calls] == ["he_bfv_noise_norm_limbs", "he_bfv_noise_norm_device"] + \
            ["he_bfv_noise_norm_limbs", "he_bfv_noise_budget_from_norm"] * B
        # the budget takes the width of the scheme's scalar, not of the slab word, and variableTime unless told otherwise
        assert calls[3] == ["he_bfv_noise_budget_from_norm", [None, scheme_bits, L, [0] * LIMBS, 1, "byref"]]
        assert result == [0.0] * B
        calls, _ = run(lambda: bfv.noise_budget_from_norm((7 << 64) | 5, 1, variable_time=False))
        assert calls[1] == ["he_bfv_noise_budget_from_norm", [None, scheme_bits, 1, [5, 7], 0, "byref"]]

        calls, result = run(lambda: bfv.is_transparent(cts(3), stream))
        assert calls == [["he_bfv_is_transparent_device", [None, word_bits, L, 3, "cts", "new0", B, "stream"]]]
        assert result == ["torch.uint8", [B], "new0"]

        calls, result = run(lambda: bfv.decrypt_workspace_bytes(B, 3, True, 1))
        assert calls == [["he_bfv_decrypt_workspace_bytes", [None, word_bits, 1, 3, 1, B]]] and result == 4096


def test_decrypt_call_shapes_8_byte_words(monkeypatch):
    _drive(monkeypatch, "BfvContext", torch.int64, 64, 64)


def test_decrypt_call_shapes_4_byte_words(monkeypatch):
    _drive(monkeypatch, "BfvContext32", torch.int32, 32, 32)


def test_decrypt_call_shapes_32_bit_scheme_on_8_byte_words(monkeypatch):
    _drive(monkeypatch, "BfvContext", torch.int64, 64, 32)


def test_signatures_have_no_suffixed_decrypt_rows():
    import heamd

    names = {name for name, _, _ in heamd.binding.SIGNATURES}
    new = {"he_bfv_decrypt_workspace_bytes", "he_bfv_secret_dot_product_device", "he_bfv_decrypt_device",
           "he_bfv_noise_norm_device", "he_bfv_is_transparent_device", "he_bfv_noise_norm_limbs",
           "he_bfv_noise_budget_from_norm"}
    assert new <= names
    assert not {name + "_u32" for name in new} & names
