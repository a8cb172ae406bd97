"""GPU tests of spasm_amd_dense_column_echelon (csrc/colechelon.hpp): the reduced column echelon form is unique, so the device is
compared byte for byte with the reference (tests/nullspace_ref.py: Python integers for the small blocks, exact numpy products for
the tall ones; tests/test_nullspace_abi.py shows the two to agree), two runs give the same bytes, and a column permutation of the
input gives the same bytes again."""
import numpy as np
import pytest

import nullspace_ref as NS
from wiedemann_ref import bal

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 257, 5000)
WIDTHS = (1, 2, 17, 64)
PRIMES3 = (3, 65521, 4294967291)


def inputs(rng, rows, k, p):
    """(name, X int32) of every kind of input at this shape"""
    full = rng.integers(0, p, size=(rows, k), dtype=np.int64)
    yield "random", bal(full, p)
    # planted: half the columns span the others, two columns are zero (raw words p and -p where they fit int32)
    r = max(1, k // 2)
    base = rng.integers(0, p, size=(rows, r), dtype=np.int64)
    mix = rng.integers(0, p, size=(r, k), dtype=np.int64)
    dep = np.zeros((rows, k), dtype=np.int64)
    for t in range(r):   # exact: one product below 2^64 is reduced at a time
        dep = (dep + NS.mulmod(np.broadcast_to(base[:, t:t + 1], dep.shape).copy(), np.broadcast_to(mix[t][None, :], dep.shape).copy(), p)) % p
    dep = bal(dep, p)
    if k > 2:
        dep[:, 0] = 0
        dep[:, k - 1] = p if p < 2**31 else 0
    yield "planted", dep
    # every pivot in the last rows
    last = np.zeros((rows, k), dtype=np.int64)
    t = min(rows, k)
    last[rows - t:] = rng.integers(1, p, size=(t, k), dtype=np.int64)
    yield "last_rows", bal(last, p)
    # the accumulator bound: words at +-halfp and the raw int32 extremes
    hp = p // 2
    ext = rng.choice(np.array([hp, -hp, 2**31 - 1, -2**31, hp - 1, 1 - hp], dtype=np.int64), size=(rows, k))
    yield "extremes", ext.astype(np.int32)


@pytest.mark.parametrize("p", PRIMES3)
@pytest.mark.parametrize("k", WIDTHS)
@pytest.mark.parametrize("rows", ROWS)
def test_column_echelon_matches_the_reference_byte_for_byte(S, rows, k, p):
    rng = np.random.default_rng(1000 * rows + 7 * k + p % 1009)
    for name, X in inputs(rng, rows, k, p):   # K > rows at rows in (1, 63) with the wide blocks
        X0 = X.copy()
        E, piv = S.column_echelon(X, p)
        assert X.tobytes() == X0.tobytes(), name
        assert E.shape == X.shape and E.dtype == np.int32
        if rows * k <= 2000:
            want, wpiv = NS.column_echelon([[int(x) for x in row] for row in X], p)
            want = bal(np.array(want, dtype=object).reshape(rows, k), p)
        else:
            want, wpiv = NS.np_column_echelon(X, p)
        assert piv.tolist() == wpiv, name
        assert E.tobytes() == want.tobytes(), name
        assert S.column_echelon(X, p)[0].tobytes() == E.tobytes(), name          # two runs
        perm = rng.permutation(k)
        E2, piv2 = S.column_echelon(np.ascontiguousarray(X[:, perm]), p)         # the same column space
        assert E2.tobytes() == E.tobytes() and piv2.tolist() == piv.tolist(), name
        # the conditions that define the form
        r = len(piv)
        assert not E[:, r:].any() and (np.diff(piv) > 0).all()
        for j, pr in enumerate(piv):
            assert E[pr, j] == 1 and not E[:pr, j].any() and np.count_nonzero(E[pr]) == 1
        assert np.abs(E.astype(np.int64)).max(initial=0) <= p // 2


def test_a_strided_block_and_the_kernel_of_a_known_space(S):
    p = 65521
    rng = np.random.default_rng(5)
    big = bal(rng.integers(0, p, size=(300, 40), dtype=np.int64), p)
    X = big[:, 3:20]                              # not contiguous: the wrapper copies
    E, piv = S.column_echelon(X, p)
    want, wpiv = NS.np_column_echelon(X, p)
    assert E.tobytes() == want.tobytes() and piv.tolist() == wpiv == list(range(17))
    # X T for an invertible T has the same column space
    T = np.triu(rng.integers(1, p, size=(17, 17), dtype=np.int64))
    XT = np.zeros((300, 17), dtype=np.int64)
    for t in range(17):
        XT = (XT + (X[:, t:t + 1].astype(np.int64) % p) * T[t][None, :]) % p
    assert S.column_echelon(bal(XT, p), p)[0].tobytes() == E.tobytes()
