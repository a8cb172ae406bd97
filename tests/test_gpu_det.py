"""GPU tests of the determinant entries (spasm_amd_det_batch / _det / _blocks_det / _dcsr_det; csrc/det.hpp).

The reference is the exact Gaussian elimination below: Python integers with pow(x, -1, p) up to n = 64, numpy int64 above (products
of two residues of a prime above 2^31 are taken in two 16-bit halves of one factor, so every intermediate stays below 2^49).
Where stated the determinant is known by construction instead: permutation matrices, scaled permutations, P * L1 * D * U1 * Q."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P16, P32 = 65521, 4294967291


# ---------------------------------------------------------------------------------------------
# the reference and the constructions
# ---------------------------------------------------------------------------------------------
def bal(v, p):
    v = int(v) % p
    return v - p if v > p // 2 else v


def perm_sign(perm):
    """+1 / -1 by cycle counting"""
    perm = [int(x) for x in perm]
    seen, cycles = [False] * len(perm), 0
    for i in range(len(perm)):
        if not seen[i]:
            cycles += 1
            while not seen[i]:
                seen[i] = True
                i = perm[i]
    return -1 if (len(perm) - cycles) % 2 else 1


def mulmod(a, b, p):
    """a * b mod p for int64 arrays of residues in [0, p), p < 2^32"""
    if p < 2**31:
        return a * b % p
    return ((a * (b >> 16) % p) * 65536 + a * (b & 0xFFFF)) % p


def host_det(D, p):
    """the determinant of the integer matrix D mod p, as a balanced residue"""
    n = len(D)
    det = 1
    if n <= 64:
        M = [[int(v) % p for v in row] for row in D]
        for c in range(n):
            i = next((i for i in range(c, n) if M[i][c]), None)
            if i is None:
                return 0
            if i != c:
                M[c], M[i] = M[i], M[c]
                det = -det
            det = det * M[c][c] % p
            inv = pow(M[c][c], -1, p)
            for k in range(c + 1, n):
                if M[k][c]:
                    f = M[k][c] * inv % p
                    M[k] = [(x - f * y) % p for x, y in zip(M[k], M[c])]
        return bal(det, p)
    M = np.array(D, dtype=np.int64) % p
    for c in range(n):
        nz = np.nonzero(M[c:, c])[0]
        if len(nz) == 0:
            return 0
        i = c + int(nz[0])
        if i != c:
            M[[c, i]] = M[[i, c]]
            det = -det
        det = det * int(M[c, c]) % p
        inv = pow(int(M[c, c]), -1, p)
        f = mulmod(M[c + 1:, c], np.int64(inv), p)
        M[c + 1:] = (M[c + 1:] - mulmod(f[:, None], M[c][None, :], p)) % p
    return bal(det, p)


def csr_raw(S, D, p):
    """the CSR of the dense integer matrix D with its non-zero entries AS THEY ARE (no reduction on the host)"""
    D = np.asarray(D, dtype=np.int64).reshape(len(D), -1 if len(D) else 0)
    n = D.shape[0]
    rows, cols = np.nonzero(D)
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ptr[1:])
    return S.CSR.from_arrays(n, n, ptr, cols, D[rows, cols], prime=p)


def csr_of(S, D, p):
    """the CSR of D mod p, balanced"""
    D = np.asarray(D, dtype=np.int64) % p
    return csr_raw(S, np.where(D > p // 2, D - p, D), p)


def perm_matrix(perm, scale=1):
    n = len(perm)
    D = np.zeros((n, n), dtype=np.int64)
    D[np.arange(n), np.asarray(perm, dtype=np.int64)] = scale
    return D


def random_dense(rng, n, p):
    return rng.integers(0, p, size=(n, n), dtype=np.int64)


def planted_dense(rng, n, p, per_row=6):
    """(D, det): D = P * L1 * Dg * U1 * Q mod p as a dense array, L1 / U1 unit triangular with about per_row entries per row and a
    full first sub- / superdiagonal (which keeps the row/column graph connected); det = sgn(P) * sgn(Q) * prod(Dg).  p < 2^31."""
    L, U = np.eye(n, dtype=np.int64), np.eye(n, dtype=np.int64)
    for i in range(n):
        for c in rng.integers(0, n, size=per_row - 2):
            if c < i:
                L[i, c] = rng.integers(1, p)
            elif c > i:
                U[i, c] = rng.integers(1, p)
        if i > 0:
            L[i, i - 1] = rng.integers(1, p)
        if i + 1 < n:
            U[i, i + 1] = rng.integers(1, p)
    dg = rng.integers(1, p, size=n, dtype=np.int64)
    M = (L * dg[None, :] % p) @ U % p
    sp, sq = rng.permutation(n), rng.permutation(n)
    det = perm_sign(sp) * perm_sign(sq)
    for v in dg.tolist():
        det = det * v % p
    return M[sp][:, sq], bal(det, p)


def planted_sparse(S, rng, n, p, per_row=6):
    """(A, det): the same construction multiplied out with CSR @ CSR"""
    def tri(lower):
        rows = []
        for i in range(n):
            cols = {int(c) for c in rng.integers(0, n, size=per_row - 1) if (c < i if lower else c > i)}
            rows.append(sorted([(c, int(rng.integers(1, p))) for c in cols] + [(i, 1)]))
        return S.CSR.from_rows(rows, n, prime=p)

    dg = [int(v) for v in rng.integers(1, p, size=n)]
    sp, sq = rng.permutation(n), rng.permutation(n)
    P = S.CSR.from_rows([[(int(c), 1)] for c in sp], n, prime=p)
    Q = S.CSR.from_rows([[(int(c), 1)] for c in sq], n, prime=p)
    Dg = S.CSR.from_rows([[(i, v)] for i, v in enumerate(dg)], n, prime=p)
    A = P @ tri(True) @ Dg @ tri(False) @ Q
    det = perm_sign(sp) * perm_sign(sq)
    for v in dg:
        det = det * v % p
    return A, bal(det, p)


# ---------------------------------------------------------------------------------------------
# the LDS kernel
# ---------------------------------------------------------------------------------------------
def test_tiny_matrices(S):
    p = P16
    mats = [
        csr_raw(S, np.zeros((0, 0)), p),                                   # the empty product
        csr_raw(S, [[-7]], p),
        csr_raw(S, [[0, 1], [1, 0]], p),
        csr_raw(S, [[p, 1], [1, 0]], p),                                   # an entry that is 0 mod p
        csr_raw(S, [[p + 5, 2 * p], [3, 2**31 - 1]], p),                   # entries above p, one of them 0 mod p
        csr_raw(S, [[-3, -p - 1], [4 - 3 * p, -(2**31) + 1]], p),          # negative entries below -p
        csr_raw(S, [[2, 0, 1], [0, 3, 0], [5, 0, 7]], 127),
    ]
    want = [1, -7, -1, -1, bal((p + 5) * (2**31 - 1), p), bal(-3 * (-(2**31) + 1) - (-p - 1) * (4 - 3 * p), p), bal(3 * (14 - 5), 127)]
    got = S.det_batch(mats)
    assert got.dtype == np.int64 and got.tolist() == want
    st = S.det_stats()
    assert st["items"] == 7 and st["lds_path"] == 7 and st["general_path"] == 0 and 1 <= st["launches"] <= 4
    assert [S.det(A) for A in mats[1:]] == want[1:]


SIGN_SIZES = [2, 3, 31, 32, 33, 63, 64, 65, 110, 111, 181]


def test_sign_alone(S):
    """permutation matrices across every class cap and the 64-lane edge of the inversion count; parities in closed form"""
    rng = np.random.default_rng(0xD371)
    mats, want = [], []
    for n in SIGN_SIZES:
        reversal = np.arange(n)[::-1]
        cycle = (np.arange(n) + 1) % n
        swap = np.arange(n)
        swap[[0, n - 1]] = swap[[n - 1, 0]]
        rnd = rng.permutation(n)
        for perm, sign in ((reversal, -1 if (n * (n - 1) // 2) % 2 else 1), (cycle, -1 if (n - 1) % 2 else 1), (swap, -1), (rnd, perm_sign(rnd))):
            mats.append(csr_raw(S, perm_matrix(perm), P16 if n % 2 else P32))
            want.append(sign)
    assert S.det_batch(mats).tolist() == want


def test_product_alone(S):
    """diag(h, .., h) times a permutation, h = (p - 1) / 2 the largest balanced magnitude"""
    rng = np.random.default_rng(0xD372)
    mats, want = [], []
    for p in (3, 127, 65521, 2147483647, 4294967291):
        h = (p - 1) // 2
        for n in (1, 64, 65, 181):
            perm = rng.permutation(n)
            mats.append(csr_raw(S, perm_matrix(perm, h), p))
            want.append(bal(perm_sign(perm) * pow(h, n, p), p))
    assert S.det_batch(mats).tolist() == want


def test_singular(S):
    rng = np.random.default_rng(0xD373)
    mats = [csr_raw(S, np.zeros((5, 5)), P16)]
    D = random_dense(rng, 40, P32)
    D[17] = D[3]
    mats.append(csr_of(S, D, P32))
    for n, p in ((33, P16), (181, P32), (181, P16)):
        D = random_dense(rng, n, p)
        D[n - 1] = D[: n - 1].sum(axis=0) % p       # rank n - 1: the deficit shows only at the last column
        mats.append(csr_of(S, D, p))
    assert S.det_batch(mats).tolist() == [0] * len(mats)


@pytest.fixture(scope="module")
def dense_batch(S):
    rng = np.random.default_rng(0xD374)
    mats, want = [], []
    for p in (P16, P32):
        for n in (5, 32, 64, 110, 181):
            D = random_dense(rng, n, p)
            mats.append(csr_of(S, D, p))
            want.append(host_det(D, p))
    return mats, want


def test_random_dense_mixed_batch(S, dense_batch):
    mats, want = dense_batch
    assert all(w != 0 for w in want)
    assert S.det_batch(mats).tolist() == want
    st = S.det_stats()
    assert st["lds_path"] == len(mats) and st["launches"] == 4


def test_deterministic(S, dense_batch):
    mats, _ = dense_batch
    a, b = S.det_batch(mats), S.det_batch(mats)
    assert a.tobytes() == b.tobytes()


def test_host_references_agree():
    """the two eliminations of this file against each other and against a construction (no device involved)"""
    rng = np.random.default_rng(0xD375)
    for n in (40, 70):                           # the Python branch, the numpy branch
        D, d = planted_dense(rng, n, P16)
        assert d != 0 and host_det(D, P16) == d
    for p in (2147483647, P32):                  # diag(D, 1): the numpy branch on the determinant the Python branch gave
        D = random_dense(rng, 64, p)
        E = np.eye(65, dtype=np.int64)
        E[:64, :64] = D
        assert host_det(D, p) == host_det(E, p) != 0


# ---------------------------------------------------------------------------------------------
# the general path, the identities
# ---------------------------------------------------------------------------------------------
def test_mixed_lds_and_general_path(S):
    rng = np.random.default_rng(0xD376)
    D4, D181 = random_dense(rng, 4, P16), random_dense(rng, 181, P16)
    A182, d182 = planted_sparse(S, rng, 182, P16)
    A300, d300 = planted_sparse(S, rng, 300, 2147483647)
    got = S.det_batch([csr_of(S, D4, P16), csr_of(S, D181, P16), A182, A300])
    st = S.det_stats()
    assert got.tolist() == [host_det(D4, P16), host_det(D181, P16), d182, d300]
    assert d182 != 0 and d300 != 0
    assert st["items"] == 4 and st["lds_path"] == 2 and st["general_path"] == 2
    # a singular matrix on the general path
    D = random_dense(rng, 190, P16)
    D[189] = D[:189].sum(axis=0) % P16
    assert S.det_batch([csr_of(S, D, P16)]).tolist() == [0]


def test_identities(S):
    n, p = 96, P16
    rng = np.random.default_rng(0xD377)
    A, B = csr_of(S, random_dense(rng, n, p), p), csr_of(S, random_dense(rng, n, p), p)
    dA, dB = S.det(A), S.det(B)
    assert dA != 0 and dB != 0
    assert [dA, dB] == S.det_batch([A, B]).tolist()
    assert S.det(A @ B) == bal(dA * dB, p)
    assert S.det(S.transpose(A)) == dA
    with S.DeviceCSR(A) as D:
        assert D.det() == dA and D.T.det() == dA
        rp, cq = rng.permutation(n), rng.permutation(n)
        assert D.permute(rp, cq).det() == bal(perm_sign(rp) * perm_sign(cq) * dA, p)
    a = 12345
    assert S.det(A * a) == bal(pow(a, n, p) * dA, p)


# ---------------------------------------------------------------------------------------------
# blocks
# ---------------------------------------------------------------------------------------------
def scrambled(S, rng, blocks, p):
    """(A, sign): the blocks on a diagonal, then row i moved to rp[i] and column j to cq[j]"""
    n = sum(b.shape[0] for b in blocks)
    assert n == sum(b.shape[1] for b in blocks)
    rp, cq = rng.permutation(n), rng.permutation(n)
    rows, r0, c0 = [None] * n, 0, 0
    for b in blocks:
        for i in range(b.shape[0]):
            rows[rp[r0 + i]] = [(int(cq[c0 + j]), int(v)) for j, v in enumerate(b[i].tolist()) if v]
        r0, c0 = r0 + b.shape[0], c0 + b.shape[1]
    return S.CSR.from_rows(rows, n, prime=p), perm_sign(rp) * perm_sign(cq)


@pytest.fixture(scope="module")
def planted_blocks():
    rng = np.random.default_rng(0xD378)
    blocks, det = [], 1
    for _ in range(100):
        D, d = planted_dense(rng, 20, P16, per_row=12)
        blocks.append(D)
        det = det * d % P16
    return blocks, det


def all_three(S, A):
    with S.DeviceBlocks(A) as Bk, S.DeviceCSR(A) as D:
        return [S.det(A), Bk.det(), S.blocks.det(Bk), D.det()], len(Bk)


def test_blocks_scrambled(S, planted_blocks):
    blocks, det = planted_blocks
    rng = np.random.default_rng(0xD379)
    A, sign = scrambled(S, rng, blocks, P16)
    assert A.n == 2000
    got, nb = all_three(S, A)
    assert nb == 100 and det != 0
    assert got == [bal(sign * det, P16)] * 4
    st = S.det_stats()
    assert st["items"] == 100 and st["lds_path"] == 100 and st["general_path"] == 0 and st["zero_by_structure"] == 0 and st["launches"] == 1
    # the host Block of the same split
    assert S.blocks.det(S.Block.from_csr(A)) == bal(sign * det, P16)


def test_blocks_not_square(S, planted_blocks):
    blocks, _ = planted_blocks
    rng = np.random.default_rng(0xD37A)
    blocks = list(blocks)
    blocks[40] = rng.integers(1, P16, size=(19, 21), dtype=np.int64)
    blocks[41] = rng.integers(1, P16, size=(21, 19), dtype=np.int64)
    A, _ = scrambled(S, rng, blocks, P16)
    got, nb = all_three(S, A)
    assert nb == 100 and got == [0] * 4
    st = S.det_stats()
    assert st["launches"] == 0 and st["zero_by_structure"] == 2 and st["lds_path"] == 0 and st["general_path"] == 0


def test_blocks_empty_row_and_column(S, planted_blocks):
    blocks, _ = planted_blocks
    rng = np.random.default_rng(0xD37B)
    A, _ = scrambled(S, rng, blocks, P16)
    rows = A.rows()
    rows[123] = []
    rows = [[(c, v) for c, v in r if c != 777] for r in rows]
    got, _ = all_three(S, S.CSR.from_rows(rows, A.n, prime=P16))
    assert got == [0] * 4
    assert S.det_stats()["launches"] == 0


def test_blocks_one_over_the_limit(S, planted_blocks):
    blocks, _ = planted_blocks
    rng = np.random.default_rng(0xD37C)
    big, dbig = planted_dense(rng, 200, P16)
    blocks = list(blocks[:57]) + [big] + list(blocks[58:])
    det = dbig
    for b in blocks[:57] + blocks[58:]:
        det = det * host_det(b, P16) % P16
    A, sign = scrambled(S, rng, blocks, P16)
    got, nb = all_three(S, A)
    assert nb == 100 and det != 0
    assert got == [bal(sign * det, P16)] * 4
    st = S.det_stats()
    assert st["general_path"] == 1 and st["lds_path"] == 99
