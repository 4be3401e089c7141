"""PolyRq<UInt32> on the device at its edges (csrc/ntt_word32.hip, the 4-byte kernels of csrc/poly_kernels.hip), bit-exact against word32_cases.py -- the CPU
oracle for the transforms, Python integers for the element-wise tables, both held to Python integers by
test_word32_cases.py:

  ntt32_kernel, ntt32_tiled_kernel   every degree 2 .. 32768 on rows of 0, p - 1, alternating, one-hot, x, half and uniform
                                     words under the three largest 30-bit primes (butterflies at the top of [0, 4p) < 2^32)
                                     and two small ones, period 5                          test_word32_every_degree
  row % mod_period, `within`         periods 1 .. 7 on 211 polynomials, generic and tiled  test_word32_row_to_modulus_map
  grids beyond one generation        1200, 300 and 10 rows at N = 8192 / 16384 / 32768     test_word32_more_rows_than_the_chip_holds
  forward, mul, inverse              a negacyclic product on 4-byte words only             test_word32_negacyclic_product
  elementwise32_kernel               all 49 pairs of {0, 1, 2, (p -+ 1) / 2, p - 2, p - 1} test_word32_elementwise_edge_table
  launch_ntt (4-byte)                N = 65536 refused, the slab untouched                 test_word32_refuses_degree_65536
"""
import numpy as np
import pytest

import heamd
import word32_cases as cases
from conftest import host_threads

pytestmark = pytest.mark.gpu

up, down = heamd.to_device32, heamd.to_host32


@pytest.mark.parametrize("degree", cases.DEGREES)
def test_word32_every_degree(oracle, degree):
    moduli, slabs = cases.edge_case(oracle, degree)
    ours = heamd.PolyContext(degree, moduli)
    for slab, forward, inverse in slabs:
        batch = slab.shape[0]
        assert np.array_equal(down(ours.forward_ntt_u32_(up(slab))), forward), batch
        assert np.array_equal(down(ours.inverse_ntt_u32_(up(slab))), inverse), batch
        assert np.array_equal(down(ours.inverse_ntt_u32_(ours.forward_ntt_u32_(up(slab)))), slab), batch
        # the 8-byte transforms of the widened slab give the same words
        assert np.array_equal(heamd.to_host(ours.forward_ntt_(heamd.to_device(slab))), forward), batch
        assert np.array_equal(heamd.to_host(ours.inverse_ntt_(heamd.to_device(slab))), inverse), batch


@pytest.mark.parametrize("period", cases.PERIODS)
@pytest.mark.parametrize("degree", cases.PERIOD_DEGREES)
def test_word32_row_to_modulus_map(oracle, degree, period):
    moduli, slab, forward, inverse = cases.period_case(oracle, degree, period, host_threads())
    ours = heamd.PolyContext(degree, moduli)
    assert np.array_equal(down(ours.forward_ntt_u32_(up(slab))), forward)
    assert np.array_equal(down(ours.inverse_ntt_u32_(up(slab))), inverse)


@pytest.mark.parametrize("degree,bits,polys", cases.CROWDED)
def test_word32_more_rows_than_the_chip_holds(oracle, degree, bits, polys):
    moduli, slab, forward = cases.crowded_case(oracle, degree, bits, polys, host_threads())
    ours = heamd.PolyContext(degree, moduli)
    evaluated = ours.forward_ntt_u32_(up(slab))
    assert np.array_equal(down(evaluated), forward)
    assert np.array_equal(down(ours.inverse_ntt_u32_(evaluated)), slab)


def test_word32_negacyclic_product(oracle):
    """test_ntt_multiplication_matches_schoolbook's shape (tests/test_gpu_ntt.py) with no 8-byte word on the way."""
    p, x, y, product = cases.product_case(oracle)
    ours = heamd.PolyContext(cases.PRODUCT_DEGREE, [p])
    evaluated = ours.elementwise_u32_("mul", ours.forward_ntt_u32_(up(x)), ours.forward_ntt_u32_(up(y)))
    assert np.array_equal(down(ours.inverse_ntt_u32_(evaluated)), product)


@pytest.mark.parametrize("degree", cases.ELEMENTWISE_DEGREES)
def test_word32_elementwise_edge_table(oracle, degree):
    moduli, lhs, rhs = cases.elementwise_case(oracle, degree)
    ours = heamd.PolyContext(degree, moduli)
    bound = np.array(moduli, dtype=np.uint64)[None, :, None]
    for op in ("add", "sub", "mul"):
        got = down(ours.elementwise_u32_(op, up(lhs), up(rhs)))
        assert (got < bound).all(), op
        assert np.array_equal(got, cases.elementwise_expected(op, moduli, lhs, rhs)), op
    got = down(ours.elementwise_u32_("neg", up(lhs)))
    assert (got < bound).all()
    assert np.array_equal(got, cases.elementwise_expected("neg", moduli, lhs))
    for scalars in cases.edge_scalars(moduli):
        got = down(ours.mul_scalar_u32_(up(lhs), scalars))
        assert (got < bound).all(), scalars
        assert np.array_equal(got, cases.elementwise_expected("mul_scalar", moduli, lhs, scalars=scalars)), scalars


def test_word32_refuses_degree_65536():
    """include/he_amd.h: "Degrees above 32768: HE_ERR_UNSUPPORTED" -- a row no longer fits the LDS.  The context itself is
    created at this degree, 4-byte tables included; the 4-byte transforms refuse before anything is enqueued."""
    degree, p = cases.REFUSED_DEGREE, cases.REFUSED_MODULUS
    ours = heamd.PolyContext(degree, [p])
    slab = np.random.default_rng(16).integers(0, p, size=(1, 1, degree), dtype=np.uint64)
    for transform in (ours.forward_ntt_u32_, ours.inverse_ntt_u32_):
        device = up(slab)
        with pytest.raises(heamd.HeError) as err:
            transform(device)
        assert err.value.code == 18 and err.value.name == "unsupportedHeOperation" and "32768" in str(err.value)
        assert np.array_equal(down(device), slab)
