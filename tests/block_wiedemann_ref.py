"""Block Wiedemann restated in plain Python integers, for the tests of spasm_amd_block_sequence, _block_berlekamp_massey and
_block_wiedemann_det: the dense block sequence, the order-by-order minimal approximant basis of [S(x); I] with its rows [g | h]
kept whole (the device keeps g and one coefficient of h), checkers for the contract (A) annihilation and (B) row-reduced, the rank
of the block Hankel matrix by dense elimination, and the determinant procedure.  No numpy arithmetic: every value is a Python int
in [0, p), converted to balanced residues only where bytes are compared."""


def balanced(x, p):
    x %= p
    return x - p if x > p // 2 else x


def mat_mul(A, B, p):
    return [[sum(a * b for a, b in zip(row, col)) % p for col in zip(*B)] for row in A]


def block_sequence(A, U, V, length, p, trans=False, d_left=None):
    """S[i][r][c] = sum_k U[k][r] * (M^i V)[k][c] mod p in [0, p), M = A, A^T, or D A / D A^T; A dense n x n, U and V n x b"""
    n = len(A)
    M = [[A[j][i] for j in range(n)] for i in range(n)] if trans else [list(r) for r in A]
    if d_left is not None:
        M = [[d_left[i] * x % p for x in M[i]] for i in range(n)]
    M = [[x % p for x in r] for r in M]
    b = len(U[0]) if n else 0
    Ut = [[U[k][r] % p for k in range(n)] for r in range(b)]
    X = [[x % p for x in row] for row in V]
    out = []
    for _ in range(length):
        out.append(mat_mul(Ut, X, p))
        X = mat_mul(M, X, p)
    return out


def approximant_basis(S, b, p):
    """The iteration of csrc/block_bm.hpp on full rows: returns (rows, deg) with rows[i] = list over t of the 2b words
    [g_i[t] | h_i[t]] and deg[i] = max(deg g_i, deg h_i + 1), at order len(S)."""
    R = 2 * b
    rows = [[[1 if c == i else 0 for c in range(R)]] for i in range(R)]
    deg = [0] * b + [1] * b
    for k in range(len(S)):
        D = []
        for i in range(R):
            d = [0] * b
            for t, w in enumerate(rows[i]):
                if t > k:
                    break
                Sk = S[k - t]
                for r in range(b):
                    if w[r]:
                        for c in range(b):
                            d[c] += w[r] * Sk[r][c]
            if k < len(rows[i]):
                for c in range(b):
                    d[c] += rows[i][k][b + c]
            D.append([x % p for x in d])
        order = sorted(range(R), key=lambda i: (deg[i], i))
        piv = [False] * R
        for s, i in enumerate(order):
            pc = next((c for c in range(b) if D[i][c]), None)
            if pc is None:
                continue
            piv[i] = True
            inv = pow(D[i][pc], p - 2, p)
            for j in order[s + 1:]:
                if D[j][pc] == 0:
                    continue
                f = (-D[j][pc] * inv) % p
                D[j] = [(x + f * y) % p for x, y in zip(D[j], D[i])]
                while len(rows[j]) < len(rows[i]):
                    rows[j].append([0] * R)
                for t, w in enumerate(rows[i]):
                    rows[j][t] = [(x + f * y) % p for x, y in zip(rows[j][t], w)]
        for i in range(R):
            if piv[i]:
                rows[i].insert(0, [0] * R)
                deg[i] += 1
    return rows, deg


def generator(S, b, p):
    """(F, rowdeg): F[t][r][c] in [0, p) for 0 <= t <= max(rowdeg), the left generator the device returns: the rows of the basis
    by ascending (degree, index) whose g(0) is independent of those already taken, reversed at their degree."""
    rows, deg = approximant_basis(S, b, p)
    order = sorted(range(2 * b), key=lambda i: (deg[i], i))
    taken, red = [], []   # red: the reduced g(0) of the rows taken, with their pivot columns
    for i in order:
        v = [x % p for x in rows[i][0][:b]]
        for w, pc in red:
            if v[pc]:
                f = (-v[pc] * pow(w[pc], p - 2, p)) % p
                v = [(x + f * y) % p for x, y in zip(v, w)]
        pc = next((c for c in range(b) if v[c]), None)
        if pc is None:
            continue
        red.append((v, pc))
        taken.append(i)
        if len(taken) == b:
            break
    assert len(taken) == b, "g(0) of an approximant basis of [S; I] has rank b"
    rowdeg = [deg[i] for i in taken]
    dmax = max(rowdeg)
    F = [[[0] * b for _ in range(b)] for _ in range(dmax + 1)]
    for r, i in enumerate(taken):
        for t in range(rowdeg[r] + 1):
            src = rowdeg[r] - t
            if src < len(rows[i]):
                F[t][r] = list(rows[i][src][:b])
    return F, rowdeg


def check_annihilates(F, rowdeg, S, p):
    """(A): for every row r and 0 <= i < len - rowdeg[r]: sum_{t <= rowdeg[r]} F_t[r, :] S_{i+t} = 0.  Also: zero above the degree."""
    b = len(rowdeg)
    for r in range(b):
        for t in range(rowdeg[r] + 1, len(F)):
            if any(x % p for x in F[t][r]):
                return False
        for i in range(len(S) - rowdeg[r]):
            for c in range(b):
                if sum(F[t][r][k] * S[i + t][k][c] for t in range(rowdeg[r] + 1) for k in range(b)) % p:
                    return False
    return True


def det_mod(M, p):
    M = [[x % p for x in r] for r in M]
    n = len(M)
    det = 1
    for c in range(n):
        pr = next((r for r in range(c, n) if M[r][c]), None)
        if pr is None:
            return 0
        if pr != c:
            M[pr], M[c] = M[c], M[pr]
            det = -det
        det = det * M[c][c] % p
        inv = pow(M[c][c], p - 2, p)
        for r in range(c + 1, n):
            if M[r][c]:
                f = M[r][c] * inv % p
                M[r] = [(x - f * y) % p for x, y in zip(M[r], M[c])]
    return det % p


def rank_mod(M, p):
    M = [[x % p for x in r] for r in M]
    rank = 0
    cols = len(M[0]) if M else 0
    for c in range(cols):
        pr = next((r for r in range(rank, len(M)) if M[r][c]), None)
        if pr is None:
            continue
        M[pr], M[rank] = M[rank], M[pr]
        inv = pow(M[rank][c], p - 2, p)
        for r in range(rank + 1, len(M)):
            if M[r][c]:
                f = M[r][c] * inv % p
                M[r] = [(x - f * y) % p for x, y in zip(M[r], M[rank])]
        rank += 1
    return rank


def leading_matrix(F, rowdeg):
    return [list(F[rowdeg[r]][r]) for r in range(len(rowdeg))]


def check_row_reduced(F, rowdeg, p):
    """(B): the matrix of leading row coefficients is non-singular"""
    return det_mod(leading_matrix(F, rowdeg), p) != 0


def block_hankel_rank(S, b, p):
    """the rank of the block Hankel matrix H[i][j] = S_{i+j} of floor((len + 1) / 2) block rows and len + 1 - that many block
    columns: the squarest one all of whose blocks are terms of the sequence, by dense elimination"""
    rows = (len(S) + 1) // 2
    cols = len(S) + 1 - rows
    H = []
    for i in range(rows):
        for r in range(b):
            H.append([S[i + j][r][c] for j in range(cols) for c in range(b)])
    return rank_mod(H, p)


def block_det(A, U, V, d, p, length):
    """(det, status) of the procedure of spasm_amd_block_wiedemann_det for one try: the block sequence of D A, its generator, and
    det A = (-1)^n det F_0 / det lc(F) / prod d when the row degrees sum to n; (0, 0) otherwise"""
    n, b = len(A), len(U[0])
    S = block_sequence(A, U, V, length, p, d_left=d)
    F, rowdeg = generator(S, b, p)
    if sum(rowdeg) != n:
        return 0, 0
    dlc = det_mod(leading_matrix(F, rowdeg), p)
    prod = 1
    for x in d:
        prod = prod * x % p
    v = det_mod(F[0], p) * pow(dlc, p - 2, p) * pow(prod, p - 2, p) % p
    if n & 1:
        v = -v % p
    return v, 1
