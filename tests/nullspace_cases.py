"""The inputs shared by tests/test_nullspace_abi.py (CPU: the Python-integer reference completes every one of them within 3 tries
at the recorded seed) and tests/test_gpu_wiedemann_kernel.py (the device must then return the same bytes): matrices, block widths,
orientations and seeds.

CASES: (name, b, trans, nullity of op(A)).  trans = 1 is run on the rectangular matrices.  One orientation is left out by a count,
not by a result: x A = 0 for the tall 40 x 30 matrix of rank 25 has nullity 15, and three tries of b = 2 form at most 6 candidates,
so that orientation is run at b = 16 only."""
import functools

import numpy as np

import wiedemann_ref as W
from block_solve_cases import dense_of   # noqa: F401  (re-exported for the tests)

P3, P16, P32 = 3, 65521, 4294967291
PRIMES = (P16, P32)
TRIES = 3

CASES = (
    ("planted30_1", 4, 0, 1),
    ("planted30_3", 4, 0, 3),
    ("wide20x33", 8, 0, 13),
    ("wide20x33", 8, 1, 0),
    ("tall40x30", 2, 0, 5),
    ("tall40x30", 16, 0, 5),
    ("tall40x30", 16, 1, 15),
    ("regular33", 8, 0, 0),
    ("zero5x6", 4, 0, 6),
    ("zero5x6", 4, 1, 5),
    ("zero1", 2, 0, 1),
    ("one1", 2, 0, 0),
    ("planted130_2", 16, 0, 2),
)
# a case starts at seed 1; a case the reference does not complete there gets another seed here (at most one case in four)
SEEDS = {}


def seed_of(name, b, trans, p):
    return SEEDS.get((name, b, trans, p), 1)


def _sparse(rng, n, m, p, per_row=5):
    D = np.zeros((n, m), dtype=np.int64)
    for i in range(n):
        cols = rng.choice(m, size=min(m, per_row), replace=False)
        D[i, cols] = rng.integers(1, p, size=len(cols))
        D[i, i % m] = int(rng.integers(1, p))
    return D


@functools.lru_cache(maxsize=None)
def matrix(name, p):
    """the matrix of a case as a wiedemann_ref.Mat"""
    rng = np.random.default_rng(sum(map(ord, name)) + p % 1009)
    if name.startswith("planted"):
        n, k = (int(x) for x in name[len("planted"):].split("_"))
        D = _sparse(rng, n, n, p)
        for j in range(k):   # the last k rows become combinations of two earlier ones
            D[n - 1 - j] = (D[2 * j] * 2 + D[2 * j + 1] * 3) % p
    elif name == "wide20x33":
        D = _sparse(rng, 20, 33, p)
    elif name == "tall40x30":
        D = _sparse(rng, 40, 30, p)
        for j in range(5):   # the last 5 columns become combinations of two earlier ones: rank 25
            D[:, 29 - j] = (D[:, 2 * j] * 2 + D[:, 2 * j + 1] * 3) % p
    elif name == "regular33":
        D = _sparse(rng, 33, 33, p)
    elif name == "zero5x6":
        D = np.zeros((5, 6), dtype=np.int64)
    elif name == "zero1":
        D = np.zeros((1, 1), dtype=np.int64)
    elif name == "one1":
        D = np.full((1, 1), 7, dtype=np.int64)
    else:
        raise KeyError(name)
    return W.Mat.from_dense(D)


def operand(name, p, trans):
    """op(A) of a case: the matrix whose right kernel is asked for"""
    M = matrix(name, p)
    return M.transpose() if trans else M


def draws(S, nr, dim, b, seed, p):
    """t -> (U, Y, d2) of try t as lists of integers in [0, p): the draws of the device"""
    def at(t):
        U, Y = S.minpoly_vectors(dim, b, seed + t, p)
        d2 = S.precond_diagonal(nr, seed + t, 0, p)
        lst = lambda a: [[int(x) % p for x in row] for row in np.asarray(a).reshape(dim, b)]
        return lst(U), lst(Y), [int(x) % p for x in d2]
    return at


def residual_is_zero(M, N, p):
    """M N = 0 mod p in exact numpy products, column by column -> list of bools"""
    Nr = np.asarray(N, dtype=np.int64).reshape(M.m, -1) % p
    if Nr.shape[1] == 0:
        return []
    MN = M.apply(Nr, p)
    return [bool((MN[:, j] == 0).all()) for j in range(MN.shape[1])]


def np_block_precond_sequence(B, U, V, length, d_left, d_right, p):
    """(length, b, b) residues in [0, p) of U^T M^i V, M = diag(d_right) B^T diag(d_left) B, by exact numpy int64 products"""
    Bt = B.transpose()
    Ur = np.asarray(U, dtype=np.int64) % p
    X = np.asarray(V, dtype=np.int64) % p
    dl = np.asarray(d_left, dtype=np.int64) % p
    dr = None if d_right is None else np.asarray(d_right, dtype=np.int64) % p
    b = Ur.shape[1]
    out = np.zeros((length, b, b), dtype=np.int64)
    for i in range(length):
        if i:
            mid = B.apply(X, p)
            mid = W.mulmod(np.broadcast_to(dl[:, None], mid.shape).copy(), mid, p)
            X = Bt.apply(mid, p)
            if dr is not None:
                X = W.mulmod(np.broadcast_to(dr[:, None], X.shape).copy(), X, p)
        for r in range(b):
            out[i, r] = W.mulmod(np.broadcast_to(Ur[:, r:r + 1], X.shape).copy(), X, p).sum(axis=0) % p
    return out
