"""GPU tests of spasm_amd_wiedemann_kernel (CSR, SpMV, DeviceCSR) and its counters.  The cases are those of
tests/nullspace_cases.py, which tests/test_nullspace_abi.py shows the Python-integer reference to complete within 3 tries at the
same seed: the device must certify them complete and return, byte for byte, the reduced column echelon form of the nullspace that
plain elimination finds.  Every returned column also passes the residual in exact numpy products.  Over GF(3), and for the matrix
with a long row (whose nullity is far beyond 64), only soundness is asserted."""
import numpy as np
import pytest

import block_wiedemann_ref as R
import nullspace_cases as K
import nullspace_ref as NS
from nullspace_cases import P3, P16, P32
from test_gpu_block_wiedemann import long_row_matrix
from wiedemann_ref import bal

pytestmark = pytest.mark.gpu


def expected(name, p, trans):
    M = K.operand(name, p, trans)
    E, piv = NS.kernel_basis(K.dense_of(M), M.m, p)
    return bal(np.array(E, dtype=object).reshape(M.m, len(piv)), p), piv


def assert_echelon(N, piv, p):
    assert N.dtype == np.int32 and N.shape[1] == len(piv) and (np.diff(piv) > 0).all()
    for j, pr in enumerate(piv):
        assert N[pr, j] == 1 and not N[:pr, j].any() and np.count_nonzero(N[pr]) == 1
    assert np.abs(N.astype(np.int64)).max(initial=0) <= p // 2


@pytest.mark.parametrize("name,b,trans,nullity", K.CASES)
@pytest.mark.parametrize("p", K.PRIMES)
def test_the_kernel_is_complete_and_equals_the_nullspace_of_elimination(S, p, name, b, trans, nullity):
    M = K.matrix(name, p)
    A = M.csr(S, p)
    seed = K.seed_of(name, b, trans, p)
    dim = M.n if trans else M.m
    N, piv, complete = S.wiedemann_kernel(A, b=b, trans=bool(trans), seed=seed, tries=K.TRIES, certify=True)
    st = S.wiedemann_kernel_stats()
    print(name, b, trans, p, st)
    assert complete is True
    assert N.shape == (dim, nullity) and len(piv) == nullity
    want, wpiv = expected(name, p, trans)
    assert piv.tolist() == wpiv and N.tobytes() == want.tobytes()
    assert all(K.residual_is_zero(K.operand(name, p, trans), N, p))
    # the counters add up
    assert (st["n"], st["m"], st["b"], st["found"], st["want"]) == (M.n, M.m, b, nullity, min(64, K.TRIES * b))
    assert st["candidates"] == b * st["tries"] and 0 <= st["accepted"] <= st["candidates"]   # rejected = candidates - accepted
    assert st["found"] == st["accepted"] - st["dependent"]
    assert st["products"] == st["sequence_products"] + st["horner_products"] + st["check_products"] + st["certify_products"]
    assert st["check_products"] == st["tries"] and st["sequence_products"] == st["tries"] * 2 * NS.block_terms(dim, b)
    if name == "wide20x33" and not trans:
        assert st["tries"] > 1
    if nullity == 0:
        assert st["tries"] == 0   # the rank bound alone decides a matrix of full column rank
    # the same bytes from two runs and through the other entry points
    assert S.wiedemann_kernel(A, b=b, trans=bool(trans), seed=seed, tries=K.TRIES, certify=True)[0].tobytes() == N.tobytes()
    with S.SpMV(A) as op:
        N2, piv2, c2 = op.wiedemann_kernel(b=b, trans=bool(trans), seed=seed, tries=K.TRIES, certify=True)
        assert (N2.tobytes(), piv2.tolist(), c2) == (N.tobytes(), piv.tolist(), True)
    with S.DeviceCSR(A) as Dv:
        N3, piv3, c3 = Dv.wiedemann_kernel(b=b, trans=bool(trans), seed=seed, tries=K.TRIES, certify=True)
        assert (N3.tobytes(), piv3.tolist(), c3) == (N.tobytes(), piv.tolist(), True)
    # without the certificate nothing is claimed and nothing else changes
    N4, piv4, c4 = S.wiedemann_kernel(A, b=b, trans=bool(trans), seed=seed, tries=K.TRIES)
    assert c4 is False and S.wiedemann_kernel_stats()["certify_products"] == 0
    # (without the bound the tries go on to the last one; they cannot add to a complete basis, and the form is unique)
    assert N4.tobytes() == N.tobytes() and piv4.tolist() == piv.tolist()


@pytest.mark.parametrize("p", K.PRIMES)
def test_want_cuts_the_basis_short(S, p):
    M = K.matrix("planted30_3", p)
    A = M.csr(S, p)
    N, piv, complete = S.wiedemann_kernel(A, want=1, b=4, seed=1, certify=True)
    assert N.shape == (30, 1) and complete is False
    assert_echelon(N, piv, p)
    assert all(K.residual_is_zero(M, N, p))
    st = S.wiedemann_kernel_stats()
    assert (st["want"], st["found"], st["accepted"], st["dependent"], st["tries"]) == (1, 1, 1, 0, 1)
    N0, piv0, complete = S.wiedemann_kernel(A, want=0, b=4, seed=1, certify=True)
    assert N0.shape == (30, 0) and complete is False
    R33 = K.matrix("regular33", p).csr(S, p)
    N0, piv0, complete = S.wiedemann_kernel(R33, want=0, b=4, seed=1, certify=True)
    assert N0.shape == (33, 0) and complete is True    # found = 0 = dim - r is proved by the rank bound


def test_the_kernel_spans_what_elimination_finds(S):
    """N against S.kernel of the same 40 x 30 matrix, whose rows k satisfy A k = 0: stacking both bases does not raise the rank"""
    p = P16
    M = K.matrix("tall40x30", p)
    A = M.csr(S, p)
    N, piv, complete = S.wiedemann_kernel(A, b=16, seed=K.seed_of("tall40x30", 16, 0, p), certify=True)
    assert complete and N.shape == (30, 5)
    Kr = S.kernel(A)
    rows = [[0] * 30 for _ in range(Kr.n)]
    for i, r in enumerate(Kr.rows()):
        for c, v in r:
            rows[i][c] = int(v) % p
    assert len(rows) == 5
    D = K.dense_of(M)
    assert not any(any(x) for x in R.mat_mul(D, [list(col) for col in zip(*rows)], p))   # A k = 0 for every row k
    both = rows + [[int(x) % p for x in col] for col in N.T]
    assert R.rank_mod(both, p) == 5 == R.rank_mod(rows, p)


@pytest.mark.parametrize("name,b,trans,nullity", [c for c in K.CASES if c[0] in ("planted30_3", "wide20x33", "tall40x30", "zero5x6", "regular33")])
def test_over_gf3_only_soundness(S, name, b, trans, nullity):
    p = P3
    M = K.matrix(name, p)
    B = K.operand(name, p, trans)
    N, piv, complete = S.wiedemann_kernel(M.csr(S, p), b=b, trans=bool(trans), seed=1, tries=3, certify=True)
    st = S.wiedemann_kernel_stats()
    print(name, b, trans, st)
    assert_echelon(N, piv, p)
    assert all(K.residual_is_zero(B, N, p))
    true_nullity = B.m - R.rank_mod(K.dense_of(B), p)
    assert N.shape[1] <= true_nullity
    if complete:
        assert N.shape[1] == true_nullity
    assert st["found"] == st["accepted"] - st["dependent"] == N.shape[1]


@pytest.mark.parametrize("trans", (False, True))
@pytest.mark.parametrize("p", K.PRIMES)
def test_segments_and_the_combine_run_under_the_composite_step(S, p, trans):
    """the long-row matrix with its last row a combination of two others: the nullity is in the thousands (empty rows and columns),
    so the basis cannot be complete; every returned column must still be a kernel vector in echelon form"""
    rng = np.random.default_rng(p % 1009)
    n = 16500
    M = long_row_matrix(rng, n, p)
    D_last = {}
    for src, f in ((3, 2), (9, 3)):   # the long row and the medium row
        for k in range(int(M.ptr[src]), int(M.ptr[src + 1])):
            D_last[int(M.j[k])] = (D_last.get(int(M.j[k]), 0) + f * int(M.v[k])) % p
    rows = [list(zip(M.j[M.ptr[i]:M.ptr[i + 1]].tolist(), M.v[M.ptr[i]:M.ptr[i + 1]].tolist())) for i in range(n - 1)]
    rows.append(sorted((c, v) for c, v in D_last.items() if v))
    M = type(M).from_rows(rows, n)
    N, piv, complete = S.wiedemann_kernel(M.csr(S, p), b=16, trans=trans, seed=1, tries=1)
    st = S.wiedemann_kernel_stats()
    print(p, trans, st)
    # the nullity is far above b = 16, so a try has kernel vectors to find: none returned would mean that the composite Horner
    # pass or the check lost them on the segments and the combine
    assert complete is False and N.shape[0] == n and 1 <= N.shape[1] <= 16
    assert_echelon(N, piv, p)
    assert all(K.residual_is_zero(M.transpose() if trans else M, N, p))
    assert st["found"] == st["accepted"] - st["dependent"] == N.shape[1] and st["candidates"] == 16
