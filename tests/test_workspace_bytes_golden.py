"""Every workspace-size function of the client layer against tests/golden/workspace_bytes.json, the table recorded from the library
of the commit before the layer's workspaces moved onto csrc/workspace_layout.hpp: the sizes are byte for byte what they were.
tests/golden/make_workspace_bytes.py says what the table holds and recomputes it; the host rows need no device, the rows of
he_simple_pir_client_workspace_bytes over real contexts (a he_simple_pir_context exists on a device only) need one."""
import collections
import importlib.util
import json
import os
import re

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FUNCTIONS_BY_WORD = ["he_bfv_encrypt_workspace_bytes", "he_bfv_decrypt_workspace_bytes", "he_pir_generate_query_workspace_bytes",
                     "he_pir_decrypt_response_workspace_bytes", "he_keyword_client_generate_query_workspace_bytes",
                     "he_keyword_client_decrypt_response_workspace_bytes", "he_keyword_client_count_entries_workspace_bytes",
                     "he_pnns_generate_query_workspace_bytes", "he_pnns_decrypt_response_workspace_bytes",
                     "he_simple_pir_client_workspace_bytes", "he_simple_pir_client_plan.a_polynomials_workspace_bytes",
                     "he_simple_pir_client_plan.encrypt_zero_workspace_bytes",
                     "he_simple_pir_client_plan.secret_times_hint_workspace_bytes",
                     "he_simple_pir_client_plan.precompute_workspace_bytes",
                     "he_simple_pir_client_plan.decrypt_responses_workspace_bytes"]
FUNCTIONS_WITHOUT_WORD = ["he_keyword_client_find_in_buckets_workspace_bytes"]


@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_workspace_bytes", os.path.join(GOLDEN, "make_workspace_bytes.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "workspace_bytes.json")) as f:
        return json.load(f)


def test_fixture_cannot_pass_on_zeros(golden):
    """at least one non-zero row per size function and per word, and a refused call (0 bytes) per function"""
    rows = {**golden["host"], **golden["device"]}
    non_zero, refused = collections.Counter(), collections.Counter()
    for key, value in rows.items():
        function = key.split("(")[0]
        word = re.search(r"word=(\d+)", key)
        non_zero[function, word.group(1) if word else None] += value != 0
        if "refused=" in key:
            assert value == 0, key
            refused[function.split(".")[0]] += 1
    for function in FUNCTIONS_BY_WORD:
        for word in ("64", "32"):
            assert non_zero[function, word] > 0, (function, word)
        assert refused[function.split(".")[0]] > 0 or function.startswith("he_simple_pir_client_plan"), function
    for function in FUNCTIONS_WITHOUT_WORD:
        assert non_zero[function, None] > 0 and refused[function] > 0, function
    assert {key.split("(")[0] for key in rows} == set(FUNCTIONS_BY_WORD + FUNCTIONS_WITHOUT_WORD)
    # two sizes known independently of the recording: 1 and 3 ciphertexts on the 8-byte context
    encrypt = "he_bfv_encrypt_workspace_bytes(word=64, operation=2, moduli_count=2, eval_out=0, count=%d)"
    assert (rows[encrypt % 1], rows[encrypt % 3]) == (384, 1152)


def test_host_rows_are_the_recorded_ones(maker, golden, monkeypatch):
    monkeypatch.delenv("HEAMD_PNNS_CLIENT_GROUP", raising=False)
    monkeypatch.delenv("HEAMD_SIMPLE_PIR_CLIENT_ROW_BLOCK", raising=False)
    got = maker.host_rows()
    assert got.keys() == golden["host"].keys()
    assert {k: (v, golden["host"][k]) for k, v in got.items() if v != golden["host"][k]} == {}


@pytest.mark.gpu
def test_device_rows_are_the_recorded_ones(maker, golden, monkeypatch):
    monkeypatch.delenv("HEAMD_SIMPLE_PIR_CLIENT_ROW_BLOCK", raising=False)
    got = maker.device_rows()
    assert got.keys() == golden["device"].keys()
    assert {k: (v, golden["device"][k]) for k, v in got.items() if v != golden["device"][k]} == {}
