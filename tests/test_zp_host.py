"""The host compilation of csrc/zp.hpp (ZP_HD: host code reduces with it -- the Euclid of spasm_amd_poly_lcm, the rank certificate,
every input that is normalised on the host) against exact integers.  No device is needed: spasm_amd_zp_reduce_probe with
where = 0 and spasm_amd_zp_field_probe_host run plain loops on the CPU.  tests/test_gpu_zp.py runs the same cases
(tests/zp_cases.py) on the device and requires the same bytes."""
import numpy as np
import pytest
import zp_cases as Z

P32, P64, host_reduce, host_field, report = Z.P32, Z.P64, Z.host_reduce, Z.host_field, Z.report


@pytest.mark.parametrize("p", Z.REDUCE_PRIMES)
def test_host_reduce_over_its_domain(S, p):
    """zp_reduce on |x| <= min(3 * 2^51 * p, 2^62), the domain derived in the header of zp.hpp: powers of two and their neighbours,
    multiples of p plus the ends of the balanced range up to the top, +-top, 24 096 random values (Z.reduce_case).  Every result
    is THE balanced residue (Python's % on Python integers)."""
    x, want = Z.reduce_case(p)
    got = host_reduce(S, p, x)
    half, mhalf = Z.halves(p)
    assert report("host zp_reduce", p, got, want, x) == 0
    assert got.min() >= mhalf and got.max() <= half


@pytest.mark.parametrize("p", Z.EXHAUSTIVE_PRIMES)
def test_host_field_operations_every_pair(S, p):
    """mul, axpy, add, sub, neg, inverse for EVERY pair of residues (c cyclic) against numpy int64 (products below 2^20) and an
    inverse table from Python's pow(a, -1, p)."""
    a, b, c, want = Z.exhaustive_case(p)
    got = host_field(S, p, a, b, c)
    half, mhalf = Z.halves(p)
    assert report("host field", p, got, want[:, :6], a, b, c) == 0
    assert got.min() >= mhalf and got.max() <= half


@pytest.mark.parametrize("p", Z.INVERSE_PRIMES)
def test_host_every_inverse(S, p):
    a, b, c, want = Z.inverse_case(p)
    got = host_field(S, p, a, b, c)[:, 5]
    assert report("host inverse", p, got, want, a) == 0


@pytest.mark.parametrize("p", Z.LARGE_PRIMES)
def test_host_worst_case_quotients(S, p):
    """zp_mul and zp_axpy where (double)a * (double)b is inexact and the quotient's fraction is next to one half: a b congruent to
    +-halfp, +-(halfp - 1), mhalfp, and to +-1 and 0 as controls, for 20 000 random a; c in {0, +-1, halfp, mhalfp} and the c that
    puts a b + c on each of those targets (Z.quotient_case: 2.08 million vectors, expected values from Python integers)."""
    q = Z.quotient_case(p)
    got = host_field(S, p, q["a"], q["b"], q["c"])
    assert report("host quotients", p, got, q["want"], q["a"], q["b"], q["c"]) == 0


def test_probe_argument_checks_need_no_device(S):
    """Bad arguments of the host entries: an error code and a text, nothing written."""
    lib = S._abi.lib()
    x = np.array([5], dtype=np.int64)
    a = np.array([1], dtype=np.int32)
    out = np.full(6, 0x55555555, dtype=np.int32)
    for call in (lambda: lib.spasm_amd_zp_reduce_probe(2, 0, 1, x.ctypes.data_as(P64), out.ctypes.data_as(P32)),
                 lambda: lib.spasm_amd_zp_reduce_probe(0xFFFFFFFC, 0, 1, x.ctypes.data_as(P64), out.ctypes.data_as(P32)),
                 lambda: lib.spasm_amd_zp_reduce_probe(7, 2, 1, x.ctypes.data_as(P64), out.ctypes.data_as(P32)),
                 lambda: lib.spasm_amd_zp_reduce_probe(7, 0, -1, x.ctypes.data_as(P64), out.ctypes.data_as(P32)),
                 lambda: lib.spasm_amd_zp_field_probe_host(2, 1, a.ctypes.data_as(P32), a.ctypes.data_as(P32), a.ctypes.data_as(P32), out.ctypes.data_as(P32))):
        assert call() == 1
        assert "bad arguments" in S._abi.last_error()
        assert (out == 0x55555555).all()
    assert lib.spasm_amd_zp_reduce_probe(7, 0, 0, None, None) == 0 and S._abi.last_error() == ""
