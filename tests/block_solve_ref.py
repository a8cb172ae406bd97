"""The block Wiedemann solve restated in plain Python integers, on top of block_wiedemann_ref.py, for the tests of
spasm_amd_block_poly_apply and spasm_amd_block_wiedemann_solve: the transposed sequence and its left generator (a right generator
of the sequence), Gauss-Jordan on [F_0 | I], the regular and the null combinations, the block Horner run and the verdicts.  U and Z
are arguments, so a test hands it the seeded vectors of the device (S.minpoly_vectors).  Every value is a Python int in [0, p)."""
import block_wiedemann_ref as R


def block_terms(n, b):
    return 2 * -(-n // b) + 2


def transpose_terms(S):
    return [[list(col) for col in zip(*T)] for T in S]


def right_generator(S, b, p):
    """(F, rowdeg) with sum_t S[i + t] F[t][r]^T = 0 for every row r: the left generator of the transposed terms"""
    return R.generator(transpose_terms(S), b, p)


def reduce_g(G, p):
    """Gauss-Jordan on [G | I]: column by column, the first row at or below the rank with a non-zero word is swapped up, scaled to 1
    and cleared from every other row.  Returns (Rm, T, rank, pivrow) with Rm = T G reduced; rows rank .. of T span the left null
    space of G."""
    b = len(G)
    g = [[x % p for x in row] for row in G]
    t = [[1 if r == c else 0 for c in range(b)] for r in range(b)]
    pivrow = [-1] * b
    rank = 0
    for c in range(b):
        if rank == b:
            break
        piv = next((r for r in range(rank, b) if g[r][c]), None)
        if piv is None:
            continue
        g[piv], g[rank] = g[rank], g[piv]
        t[piv], t[rank] = t[rank], t[piv]
        inv = pow(g[rank][c], p - 2, p)
        g[rank] = [x * inv % p for x in g[rank]]
        t[rank] = [x * inv % p for x in t[rank]]
        for r in range(b):
            f = g[r][c]
            if r != rank and f:
                g[r] = [(x - f * y) % p for x, y in zip(g[r], g[rank])]
                t[r] = [(x - f * y) % p for x, y in zip(t[r], t[rank])]
        pivrow[c] = rank
        rank += 1
    return g, t, rank, pivrow


def combinations(F, p, ncols):
    """[(regular, h)] for the columns 0 .. ncols - 1 of V: h[t] = lambda F[t] (b words), lambda F[0] = e_j where e_j lies in the row
    space of F[0] (regular), else lambda the (j mod nullity)-th left null vector of F[0] in the order reduce_g leaves them"""
    b = len(F[0])
    g, t, rank, pivrow = reduce_g(F[0], p)
    out = []
    for j in range(ncols):
        pr = pivrow[j]
        regular = pr >= 0 and g[pr] == [1 if k == j else 0 for k in range(b)]
        lam = t[pr] if regular else t[rank + j % (b - rank)]
        h = [[sum(lam[r] * Ft[r][c] for r in range(b)) % p for c in range(b)] for Ft in F]
        assert h[0] == ([1 if k == j else 0 for k in range(b)] if regular else [0] * b)
        out.append((regular, h))
    return out


def horner_table(combos, D, p):
    """C[s][c][j] = -h_j[s + 1][c] for 0 <= s < D: what spasm_amd_block_poly_apply takes as coef with its D = D - 1"""
    b = len(combos[0][1][0])
    return [[[(-h[s + 1][c]) % p if s + 1 < len(h) else 0 for _, h in combos] for c in range(b)] for s in range(D)]


def block_poly_apply(M, C, V, p):
    """X = sum_t M^t V C[t] by block Horner: M dense n x n, V n x b, C a list of b x K matrices; [] gives zeros (K unknown: [])"""
    n = len(M)
    if not C:
        return [[] for _ in range(n)]
    Vp = [[x % p for x in row] for row in V]
    Y = None
    for Cs in reversed(C):
        VC = R.mat_mul(Vp, Cs, p) if n else []
        Y = VC if Y is None else [[(a + c) % p for a, c in zip(ra, rc)] for ra, rc in zip(R.mat_mul(M, Y, p), VC)]
    return Y


def solve_try(M, B, U, Z, p, seq=None):
    """One try of spasm_amd_block_wiedemann_solve for the n x K right-hand sides B (K <= b) with the try's vectors U, Z (n x b):
    returns (X, status, info), X n x K in [0, p), status per column 1 / 2 / 0 (the column of X is zero then).  M is op(A), dense.
    seq: the block sequence of U, [B | Z] when the caller has it already (block_terms(n, b) terms)."""
    n, b, K = len(M), len(U[0]), len(B[0])
    M = [[x % p for x in row] for row in M]
    V = [[x % p for x in (list(B[r]) + list(Z[r][K:]))] for r in range(n)]
    S = seq if seq is not None else R.block_sequence(M, U, V, block_terms(n, b), p)
    F, rowdeg = right_generator(S, b, p)
    D = max(rowdeg)
    combos = combinations(F, p, K)
    X = block_poly_apply(M, horner_table(combos, D, p), V, p) if D else [[0] * K for _ in range(n)]
    MX = R.mat_mul(M, X, p)
    status = []
    for j, (regular, _) in enumerate(combos):
        res = [(MX[r][j] - (V[r][j] if regular else 0)) % p for r in range(n)]
        rzero, xzero = not any(res), not any(X[r][j] for r in range(n))
        st = 1 if regular and rzero else 2 if (not regular and rzero and not xzero) else 0
        status.append(st)
        if st == 0:
            for r in range(n):
                X[r][j] = 0
    return X, status, {"rowdeg": rowdeg, "D": D, "regular": [c[0] for c in combos], "len": len(S)}


def solve_dense(M, bvec, p):
    """the unique solution of M x = bvec mod p by elimination, or None when M is singular"""
    n = len(M)
    A = [[x % p for x in row] + [bvec[i] % p] for i, row in enumerate(M)]
    for c in range(n):
        pr = next((r for r in range(c, n) if A[r][c]), None)
        if pr is None:
            return None
        A[pr], A[c] = A[c], A[pr]
        inv = pow(A[c][c], p - 2, p)
        A[c] = [x * inv % p for x in A[c]]
        for r in range(n):
            if r != c and A[r][c]:
                f = A[r][c]
                A[r] = [(x - f * y) % p for x, y in zip(A[r], A[c])]
    return [A[r][n] for r in range(n)]
