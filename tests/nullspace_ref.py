"""Kernel bases restated in plain Python integers, for the tests of spasm_amd_dense_column_echelon, _block_precond_sequence and
_wiedemann_kernel: the reduced column echelon form column by column as csrc/colechelon.hpp does it, the nullspace by plain
elimination, and one try of the kernel routine on top of the generator of block_wiedemann_ref.py.  The draws (U, Y, D2) are
arguments, so a test hands it those of the device (S.minpoly_vectors, S.precond_diagonal).  Every value is a Python int in [0, p).
np_column_echelon is the same form in exact numpy int64 products, for blocks too tall for a Python loop; the CPU tests show the
two to agree."""
import numpy as np

import block_wiedemann_ref as R
from wiedemann_ref import bal, mulmod


def block_terms(dim, b):
    return 2 * -(-dim // b) + 2


def column_echelon(X, p):
    """(E, pivots): X a list of rows of K integers.  Column by column: the first row with a non-zero word is the pivot, the column
    is scaled to a 1 there and cleared from that row of every other column; the columns with a pivot are then sorted by it and
    the others are zero."""
    E = [[x % p for x in row] for row in X]
    K = len(E[0]) if E else 0
    piv = []
    for c in range(K):
        pr = next((r for r in range(len(E)) if E[r][c]), None)
        if pr is None:
            continue
        inv = pow(E[pr][c], p - 2, p)
        m = list(E[pr])
        for row in E:
            xc = row[c] * inv % p
            if xc == 0 and row[c] == 0:
                continue
            for j in range(K):
                row[j] = xc if j == c else (row[j] - xc * m[j]) % p
        piv.append((pr, c))
    piv.sort()
    out = [[row[c] for _, c in piv] + [0] * (K - len(piv)) for row in E]
    return out, [r for r, _ in piv]


def np_column_echelon(X, p):
    """the same form for an integer array (rows, K) -> (balanced int32 array, pivots)"""
    E = np.asarray(X, dtype=np.int64) % p
    rows, K = E.shape
    piv = []
    for c in range(K):
        nz = np.flatnonzero(E[:, c])
        if not len(nz):
            continue
        pr = int(nz[0])
        inv = pow(int(E[pr, c]), p - 2, p)
        m = E[pr].copy()
        xc = mulmod(E[:, c].copy(), np.full(rows, inv, dtype=np.int64), p)
        E = (E - mulmod(np.broadcast_to(xc[:, None], E.shape).copy(), np.broadcast_to(m[None, :], E.shape).copy(), p)) % p
        E[:, c] = xc
        piv.append((pr, c))
    piv.sort()
    out = np.zeros_like(E)
    for j, (_, c) in enumerate(piv):
        out[:, j] = E[:, c]
    return bal(out, p), [r for r, _ in piv]


def rref(M, p):
    """the reduced row echelon form of M by Gauss-Jordan, zero rows dropped, and its pivot columns"""
    M = [[x % p for x in row] for row in M]
    cols = len(M[0]) if M else 0
    rank, pivots = 0, []
    for c in range(cols):
        pr = next((r for r in range(rank, len(M)) if M[r][c]), None)
        if pr is None:
            continue
        M[pr], M[rank] = M[rank], M[pr]
        inv = pow(M[rank][c], p - 2, p)
        M[rank] = [x * inv % p for x in M[rank]]
        for r in range(len(M)):
            if r != rank and M[r][c]:
                f = M[r][c]
                M[r] = [(x - f * y) % p for x, y in zip(M[r], M[rank])]
        pivots.append(c)
        rank += 1
    return M[:rank], pivots


def nullspace(B, dim, p):
    """a basis of {x : B x = 0} by plain elimination, as the columns of a dim x nullity list of rows: one vector per free column"""
    Rm, pivots = rref(B, p) if B else ([], [])
    free = [c for c in range(dim) if c not in pivots]
    N = [[0] * len(free) for _ in range(dim)]
    for k, f in enumerate(free):
        N[f][k] = 1
        for r, pc in enumerate(pivots):
            N[pc][k] = -Rm[r][f] % p
    return N


def kernel_basis(B, dim, p):
    """(E, pivots): the reduced column echelon form of the whole kernel of B (rows of dim integers); E is dim x nullity"""
    N = nullspace(B, dim, p)
    if not N or not N[0]:
        return [[] for _ in range(dim)], []
    return column_echelon(N, p)


def composite(B, d2, p):
    """M = B^T diag(d2) B, dense dim x dim"""
    dim = len(B[0])
    DB = [[d2[i] * x % p for x in row] for i, row in enumerate(B)]
    Bt = [[B[i][j] % p for i in range(len(B))] for j in range(dim)]
    return R.mat_mul(Bt, DB, p)


def kernel_try(B, U, Y, d2, p):
    """One try of spasm_amd_wiedemann_kernel for B = op(A) (nr x dim, dense): V = M Y, the block sequence of M on U, V, the left
    generator F of its transposed terms, the candidates W = sum_s M^s Y F_s^T by Horner over Y, and the residual B W.  Returns
    (W, accepted): W dim x b, accepted the columns with a zero residual that are not zero."""
    dim, b = len(Y), len(Y[0])
    M = composite(B, d2, p)
    Yp = [[x % p for x in row] for row in Y]
    V = R.mat_mul(M, Yp, p)
    S = R.block_sequence(M, U, V, block_terms(dim, b), p)
    F, rowdeg = R.generator([[list(col) for col in zip(*T)] for T in S], b, p)
    Wm = None
    for Fs in reversed(F):
        YC = R.mat_mul(Yp, [list(col) for col in zip(*Fs)], p)   # C_s = F_s^T
        Wm = YC if Wm is None else [[(a + c) % p for a, c in zip(ra, rc)] for ra, rc in zip(R.mat_mul(M, Wm, p), YC)]
    BW = R.mat_mul([[x % p for x in row] for row in B], Wm, p)
    accepted = [j for j in range(b) if not any(row[j] for row in BW) and any(row[j] for row in Wm)]
    return Wm, accepted


def kernel(B, dim, b, p, draws, tries=3, want=None, target=None):
    """The loop of spasm_amd_wiedemann_kernel: draws(t) -> (U, Y, d2) of try t.  target: dim - r of the certificate (None: no
    certificate).  Returns (E, pivots, complete, info), E dim x found in [0, p)."""
    want = min(64, tries * b) if want is None else want
    basis, pivots = [[] for _ in range(dim)], []
    info = {"tries": 0, "candidates": 0, "accepted": 0, "dependent": 0}
    for t in range(tries):
        have = len(pivots)
        if have >= want or (target is not None and have == target):
            break
        U, Y, d2 = draws(t)
        Wm, acc = kernel_try(B, U, Y, d2, p)
        take = acc[: want - have]
        info["tries"] = t + 1
        info["candidates"] += b
        if not take:
            continue
        E, pivots = column_echelon([basis[r] + [Wm[r][j] for j in take] for r in range(dim)], p)
        basis = [row[: len(pivots)] for row in E]
        info["accepted"] += len(take)
        info["dependent"] += have + len(take) - len(pivots)
    return basis, pivots, target is not None and len(pivots) == target, info
