"""The plain-slab transform pair at N = 8192 on the signed shift-folded butterflies (ntt_common.hpp kModeFoldSigned) against the
CPU oracle, word for word -- never against the GPU path itself.

Two launch shapes per context: one polynomial (the one-row-per-workgroup kernel) and the smallest launch that takes the
row-pair kernel, one polynomial more than kUngroupedBelowRows = 4096 rows (L = 4: 1 025 polynomials, 4 100 rows, 256 MiB).
Inputs: all p - 1 (every difference and every sum at its extreme), all 0, alternating 0 / p - 1, a single p - 1 at index 0 and
another at index N - 1, seeded uniform residues.  Contexts: the benchmark's four 55-bit primes, and L = 1 on the smallest
modulus that takes these butterflies at this degree (a prime 1 mod 2N lies at least 2N - 1 below its power of two, so the
41-bit edge of the products has no prime here; that edge is covered by tests/test_gpu_fold_signed_probe.py)."""
import numpy as np
import pytest

import fold_signed_model as M
import heamd

pytestmark = pytest.mark.gpu

DEGREE = 8192
UNGROUPED_BELOW_ROWS = 4096  # ntt_policy.hpp kUngroupedBelowRows
ORACLE_THREADS = 16
INPUTS = ["all_p_minus_1", "all_zero", "alternating", "two_spikes", "uniform"]


def _smallest_eligible(oracle):
    for bits in range(41, 56):
        p = int(oracle.generate_primes([bits], False, DEGREE)[0])
        if M.eligible(p):
            return p
    raise AssertionError("no eligible modulus")


@pytest.fixture(scope="module")
def contexts(oracle):
    out = {}
    for name, moduli in (("benchmark", [int(p) for p in oracle.generate_primes([55, 55, 55, 55], False, DEGREE)]),
                         ("smallest", [_smallest_eligible(oracle)])):
        assert all(M.eligible(p) for p in moduli), moduli
        out[name] = (moduli, heamd.PolyContext(DEGREE, moduli), oracle.PolyContext(DEGREE, moduli))
    return out


def _polynomial(kind, moduli):
    """one polynomial [L, N] of the structured inputs"""
    top = np.array([p - 1 for p in moduli], dtype=np.uint64).reshape(-1, 1)
    x = np.zeros((len(moduli), DEGREE), dtype=np.uint64)
    if kind == "all_p_minus_1":
        x[:] = top
    elif kind == "alternating":
        x[:, 1::2] = top
    elif kind == "two_spikes":
        x[:, 0] = top[:, 0]
        x[:, DEGREE - 1] = top[:, 0]
    else:
        assert kind == "all_zero"
    return x


def _slab(kind, moduli, polys):
    """-> (the launch's slab [polys, L, N], the distinct polynomials the oracle has to transform)"""
    if kind == "uniform":
        rng = np.random.default_rng(8192 + polys + len(moduli))
        rows = [rng.integers(0, p, size=(polys, DEGREE), dtype=np.uint64) for p in moduli]
        slab = np.ascontiguousarray(np.stack(rows, axis=1))
        return slab, slab
    one = _polynomial(kind, moduli)[None]
    return np.ascontiguousarray(np.broadcast_to(one, (polys,) + one.shape[1:])), one


def _same(got, expected):
    return np.array_equal(got, np.broadcast_to(expected, got.shape))


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("pairs", [False, True], ids=["one_polynomial", "row_pairs"])
@pytest.mark.parametrize("name", ["benchmark", "smallest"])
def test_transforms_match_the_oracle(contexts, name, pairs, kind):
    moduli, ours, ref = contexts[name]
    polys = UNGROUPED_BELOW_ROWS // len(moduli) + 1 if pairs else 1
    assert (polys * len(moduli) > UNGROUPED_BELOW_ROWS) == pairs
    slab, distinct = _slab(kind, moduli, polys)
    forward = ref.forward_ntt(distinct, threads=ORACLE_THREADS)
    inverse = ref.inverse_ntt(distinct, threads=ORACLE_THREADS)
    round_trip = ref.inverse_ntt(forward, threads=ORACLE_THREADS)
    dev = heamd.to_device(slab)
    assert _same(heamd.to_host(ours.forward_ntt_(dev)), forward), "forward"
    assert _same(heamd.to_host(ours.inverse_ntt_(dev)), round_trip), "forward then inverse"
    assert _same(heamd.to_host(ours.inverse_ntt_(heamd.to_device(slab))), inverse), "inverse"
