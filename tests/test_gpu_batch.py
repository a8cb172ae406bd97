"""GPU tests of the batched entries (spasm_amd_echelonize_batch / _rank_batch / _kernel_batch; csrc/batch.hpp).

The independent check is the exact reduced row echelon form computed below on the host in integer arithmetic (int64 while every
product stays below 2^62, i.e. for primes below 2^31; Python integers in numpy object arrays above).  The batch is also
compared with the per-matrix engine under LM (leftmost-entry pivots) and with the oracle."""
import hashlib
import os

import numpy as np
import pytest
from conftest import LM

pytestmark = pytest.mark.gpu

PRIMES = [3, 7, 127, 251, 42013, 65521, 2147483647, 4294967291]
LIMIT = 32768


# ---------------------------------------------------------------------------------------------
# the reference: exact RREF on the host
# ---------------------------------------------------------------------------------------------
def host_rref(D, p):
    """(R, pivot columns): the reduced row echelon form of D mod p (residues in [0, p)), zero rows dropped.  Columns left to right,
    the pivot of a column is the first row below the pivots found so far that holds it (after the swaps of plain Gauss-Jordan):
    the pivot COLUMNS and the reduced form do not depend on that choice."""
    big = p >= 2**31
    M = np.array(D, dtype=object if big else np.int64) % p
    n, m = M.shape
    piv, r = [], 0
    for c in range(m):
        if r == n:
            break
        nzr = [i for i in range(r, n) if M[i, c] != 0]
        if not nzr:
            continue
        i = nzr[0]
        if i != r:
            M[[r, i]] = M[[i, r]]
        M[r] = (M[r] * pow(int(M[r, c]), -1, p)) % p
        for k in range(n):
            if k != r and M[k, c] != 0:
                M[k] = (M[k] - M[k, c] * M[r]) % p
        piv.append(c)
        r += 1
    return M[:r], piv


def balanced_rows(M, p):
    """rows of a residue matrix as sorted lists of (column, balanced value)"""
    out = []
    for row in M:
        out.append([(j, int(v) - p if int(v) > p // 2 else int(v)) for j, v in enumerate(row) if int(v) != 0])
    return out


def to_csr(S, D, p, rng=None):
    """the CSR of the dense residue matrix D (n x m); with rng, the entries of each row in a shuffled (unsorted) order"""
    n, m = D.shape
    rows = []
    for i in range(n):
        cols = [j for j in range(m) if int(D[i, j]) % p != 0]
        if rng is not None:
            cols = [cols[k] for k in rng.permutation(len(cols))]
        rows.append([(j, int(D[i, j])) for j in cols])
    return S.CSR.from_rows(rows, m, prime=p)


def random_dense(rng, n, m, p, density, deficiency=0, zero_rows=0, zero_cols=0):
    D = np.zeros((n, m), dtype=object)
    mask = rng.random((n, m)) < density
    vals = rng.integers(1, p, size=(n, m))
    D[mask] = vals[mask]
    D = D.astype(object)
    for _ in range(deficiency):  # planted dependencies: a row becomes a combination of two others
        if n >= 3:
            a, b, c = (int(v) for v in rng.choice(n, size=3, replace=False))
            D[a] = (int(rng.integers(1, p)) * D[b] + int(rng.integers(1, p)) * D[c]) % p
    for _ in range(zero_rows):
        D[int(rng.integers(0, n))] = 0
    for _ in range(zero_cols):
        D[:, int(rng.integers(0, m))] = 0
    return D


def sweep_cases():
    """about 300 seeded (n, m, prime, density, deficiency, zero rows, zero columns), all inside the LDS limit"""
    rng = np.random.default_rng(20240611)
    cases = []
    # the corners: 1 x 1, one row, one column, the limit tall / wide / square, each once per a few primes
    corners = [(1, 1), (1, 2), (2, 1), (1, 300), (300, 1), (128, 256), (256, 128), (181, 181), (64, 512), (512, 64), (2, 16384), (16384, 2), (5, 6000)]
    for k, (n, m) in enumerate(corners):
        p = PRIMES[(3 * k + 2) % len(PRIMES)]
        big = n * m > 20000
        cases.append((n, m, p, 0.05 if big else 0.6, 2 if n >= 3 else 0, 1 if n > 4 else 0, 1 if m > 4 else 0))
    cases.append((128, 256, 65521, 1.0, 0, 0, 0))
    cases.append((100, 100, 4294967291, 1.0, 3, 0, 0))
    cases.append((90, 120, 2147483647, 1.0, 2, 1, 1))
    while len(cases) < 300:
        kind = len(cases) % 3
        a, b = int(rng.integers(1, 48)), int(rng.integers(1, 48))
        n, m = (max(a, b) + 8, min(a, b)) if kind == 0 else ((min(a, b), max(a, b) + 8) if kind == 1 else (a, a))
        if len(cases) % 25 == 0:
            n, m = n * 3, m * 3
        p = PRIMES[int(rng.integers(0, len(PRIMES)))]
        density = float(rng.choice([0.02, 0.05, 0.1, 0.3, 0.6, 1.0]))
        cases.append((n, m, p, density, int(rng.integers(0, 3)), int(rng.integers(0, 2)), int(rng.integers(0, 2))))
    return cases


@pytest.fixture(scope="module")
def sweep(S):
    rng = np.random.default_rng(77)
    mats, dense = [], []
    for (n, m, p, density, deficiency, zr, zc) in sweep_cases():
        assert n * m <= LIMIT
        D = random_dense(rng, n, m, p, density, deficiency, zr, zc)
        dense.append((D, p))
        mats.append(to_csr(S, D, p, rng))
    # a matrix without rows and one without entries
    mats.append(S.CSR.from_rows([], 7, prime=127))
    dense.append((np.zeros((0, 7), dtype=object), 127))
    mats.append(S.CSR.from_rows([[], [], []], 5, prime=42013))
    dense.append((np.zeros((3, 5), dtype=object), 42013))
    return mats, dense


def lu_bytes(fact):
    U = fact.U
    nz = int(U.p[U.n])
    return (fact.r, U.p.tobytes(), U.j[:nz].tobytes(), U.x[:nz].tobytes(), np.asarray(fact.qinv).tobytes(), np.asarray(fact.p).tobytes())


def test_sweep_against_host_rref_engine_and_oracle(S, O, sweep):
    mats, dense = sweep
    facts = S.echelonize_batch(mats)
    st = S.batch_stats()
    print("batch_stats", st)
    # the path actually taken: every matrix of the sweep is inside the limit
    assert st["matrices"] == len(mats) and st["lds_path"] == len(mats) and st["general_path"] == 0
    assert st["chunks"] >= 1 and st["launches"] <= 6 * st["chunks"] and st["max_image_words"] <= 34816
    assert S._abi.last_error() == ""
    digest = hashlib.sha256(b"batch sweep").digest()
    for idx, (A, (D, p), fact) in enumerate(zip(mats, dense, facts)):
        where = f"matrix {idx}: {A.n} x {A.m} mod {p}"
        R, piv = host_rref(D, p)
        one = S.echelonize(A, **LM)
        assert fact.r == len(piv) == one.r == O.echelonize(A, **LM).r, where
        qinv = np.asarray(fact.qinv)
        assert [j for j in range(A.m) if qinv[j] >= 0] == piv, where
        assert [int(qinv[j]) for j in piv] == list(range(len(piv))), where
        # the documented shape of the LU
        assert fact.U.shape == (fact.r, A.m) and not fact.complete and not fact.data.contents.L, where
        pp = np.ctypeslib.as_array(fact.data.contents.p, (max(A.n, A.m, 1),))
        assert sorted(pp[: A.n].tolist()) == list(range(A.n)) and sorted(pp[fact.r: A.n].tolist()) == pp[fact.r: A.n].tolist(), where
        want = balanced_rows(R, p)
        assert fact.U.rows() == want, where  # U is the reduced form itself, row k on the k-th pivot column
        assert sorted(S.rref(fact)[0].rows()) == sorted(want), where
        assert sorted(S.kernel(fact).rows()) == sorted(S.kernel(one).rows()), where
        assert S.factorization_verify(A, fact, 1000 + idx), where
        proof = S.certificate_rank_create(A, digest, fact)
        assert proof.r == fact.r and S.certificate_rank_verify(A, digest, proof), where


def test_rank_and_kernel_batches(S, sweep):
    mats, _ = sweep
    facts = S.echelonize_batch(mats)
    assert S.rank_batch(mats) == [f.r for f in facts]
    st = S.batch_stats()
    assert st["lds_path"] == len(mats) and st["general_path"] == 0 and st["entries"] == 0 and st["chunks"] == 1
    Ks = S.kernel_batch(mats)
    st = S.batch_stats()
    assert st["lds_path"] == len(mats) and st["general_path"] == 0
    for A, fact, K in zip(mats, facts, Ks):
        assert K.shape == (A.m - fact.r, A.m) and K.prime == A.prime
        assert K.rows() == S.kernel(fact).rows(), (A.n, A.m, A.prime)
        free = [j for j in range(A.m) if fact.qinv[j] < 0]
        assert [row[-1] for row in K.rows()] == [(f, -1) for f in free]  # ascending order of the free column


def host_elected_rows(D, p):
    """the rows in the order the election takes them: per column, left to right, the first row that is not a pivot yet and holds a
    non-zero there once the pivots before it are eliminated (Gauss-Jordan without swaps, Python integers)"""
    M = [[int(v) % p for v in row] for row in np.asarray(D, dtype=object)]
    taken = []
    for c in range(len(M[0]) if M else 0):
        i = next((i for i in range(len(M)) if i not in taken and M[i][c]), None)
        if i is None:
            continue
        inv = pow(M[i][c], -1, p)
        for k in range(len(M)):
            if k != i and M[k][c]:
                f = M[k][c] * inv % p
                M[k] = [(a - f * b) % p for a, b in zip(M[k], M[i])]
        taken.append(i)
    return taken


def test_wide_matrices_end_their_qinv_with_minus_one(S):
    """Every row is a pivot before the columns run out, so the elimination stops early and the columns left have no pivot: full row
    rank at 1 x 33, 3 x 40, 2 x 65 (past a bitset word, past a wave) and 5 x 6, and a 4 x 40 of rank 2."""
    rng = np.random.default_rng(3365)
    mats, dense = [], []
    for p in (65521, 127):
        for (n, m) in ((1, 33), (3, 40), (2, 65), (5, 6)):
            while True:
                D = random_dense(rng, n, m, p, 0.7)
                piv = host_rref(D, p)[1]
                if len(piv) == n and piv[-1] < m - 1:
                    break
            dense.append((D, p))
    D = random_dense(rng, 4, 40, 65521, 0.7)
    D[1] = (3 * D[0]) % 65521
    D[3] = (D[0] + 5 * D[2]) % 65521
    assert len(host_rref(D, 65521)[1]) == 2 and host_rref(D, 65521)[1][-1] < 39
    dense.append((D, 65521))
    mats = [to_csr(S, D, p, rng) for D, p in dense]
    facts = S.echelonize_batch(mats)
    st = S.batch_stats()
    assert st["lds_path"] == len(mats) and st["general_path"] == 0
    ranks = S.rank_batch(mats)
    Ks = S.kernel_batch(mats)
    for A, (D, p), fact, rank, K in zip(mats, dense, facts, ranks, Ks):
        where = f"{A.n} x {A.m} mod {p}"
        R, piv = host_rref(D, p)
        r = len(piv)
        assert fact.r == rank == r, where
        want_qinv = [-1] * A.m
        for k, c in enumerate(piv):
            want_qinv[c] = k
        assert np.asarray(fact.qinv).tolist() == want_qinv and want_qinv[-1] == -1, where
        elected = host_elected_rows(D, p)
        pp = np.ctypeslib.as_array(fact.data.contents.p, (max(A.n, A.m, 1),))
        assert pp[: A.n].tolist() == elected + [i for i in range(A.n) if i not in elected], where
        want = balanced_rows(R, p)
        assert fact.U.rows() == want, where
        free = [f for f in range(A.m) if f not in piv]
        assert K.shape == (A.m - r, A.m), where
        assert K.rows() == [[(piv[k], v) for k in range(r) for (j, v) in want[k] if j == f] + [(f, -1)] for f in free], where


def test_mixed_batch_takes_the_general_path_where_it_must(S, sweep):
    mats, dense = sweep
    rng = np.random.default_rng(5)
    over = [(200, 200, 65521), (10, 4000, 127), (33000, 1, 42013)]
    big = [to_csr(S, random_dense(rng, n, m, p, 0.02 if n * m > 30000 and m > 1 else 0.5, 2), p, rng) for (n, m, p) in over]
    batch = mats[:20] + [big[0]] + mats[20:40] + [big[1], big[2]]
    slow = {20, 41, 42}
    facts = S.echelonize_batch(batch, **LM)
    st = S.batch_stats()
    assert st["matrices"] == len(batch) and st["general_path"] == 3 and st["lds_path"] == len(batch) - 3
    ranks = S.rank_batch(batch, **LM)
    assert S.batch_stats()["general_path"] == 3
    Ks = S.kernel_batch(batch, **LM)
    assert S.batch_stats()["general_path"] == 3
    for i, (A, fact, K) in enumerate(zip(batch, facts, Ks)):
        one = S.echelonize(A, **LM)
        assert fact.r == one.r == ranks[i]
        assert sorted(S.rref(fact)[0].rows()) == sorted(S.rref(one)[0].rows())
        assert sorted(K.rows()) == sorted(S.kernel(one).rows())
        if i in slow:  # the per-matrix call itself
            assert fact.U.rows() == one.U.rows() and np.array_equal(fact.qinv, one.qinv)
    # a call that asks for L: every matrix through the general path, with its L
    few = mats[:6]
    withL = S.echelonize_batch(few, L=True, **LM)
    st = S.batch_stats()
    assert st["general_path"] == len(few) and st["lds_path"] == 0 and st["launches"] == 0
    for A, fact in zip(few, withL):
        one = S.echelonize(A, L=True, **LM)
        assert fact.r == one.r and fact.U.rows() == one.U.rows() and fact.L.shape == one.L.shape
        assert S.factorization_verify(A, fact, 3)


def test_batch_is_deterministic(S, sweep):
    mats, _ = sweep
    a = [lu_bytes(f) for f in S.echelonize_batch(mats)]
    b = [lu_bytes(f) for f in S.echelonize_batch(mats)]
    assert a == b
    ka = [(K.p.tobytes(), K.j[: int(K.p[K.n])].tobytes(), K.x[: int(K.p[K.n])].tobytes()) for K in S.kernel_batch(mats)]
    kb = [(K.p.tobytes(), K.j[: int(K.p[K.n])].tobytes(), K.x[: int(K.p[K.n])].tobytes()) for K in S.kernel_batch(mats)]
    assert ka == kb


def test_small_scratch_budget_cuts_the_batch_into_chunks(S, sweep, monkeypatch):
    mats, _ = sweep
    whole = [lu_bytes(f) for f in S.echelonize_batch(mats)]
    assert S.batch_stats()["chunks"] == 1
    kwhole = [K.rows() for K in S.kernel_batch(mats)]
    monkeypatch.setenv("SPASM_AMD_BATCH_SCRATCH_MB", "1")
    cut = [lu_bytes(f) for f in S.echelonize_batch(mats)]
    st = S.batch_stats()
    print("batch_stats", st)
    assert st["chunks"] > 3 and st["lds_path"] == len(mats) and st["launches"] <= 6 * st["chunks"]
    assert cut == whole
    assert [K.rows() for K in S.kernel_batch(mats)] == kwhole and S.batch_stats()["chunks"] > 3
    monkeypatch.delenv("SPASM_AMD_BATCH_SCRATCH_MB")
    S.echelonize_batch(mats[:3])
    assert S.batch_stats()["chunks"] == 1


def block_matrix(S, ncomp, seed, p=42013):
    """ncomp independent blocks of mixed small shapes, each connected and rank deficient, rows and columns interleaved, plus an
    isolated empty row and an isolated empty column"""
    rng = np.random.default_rng(seed)
    shapes = [(int(rng.integers(2, 14)), int(rng.integers(2, 14))) for _ in range(ncomp)]
    n = sum(a for a, _ in shapes) + 1
    m = sum(b for _, b in shapes) + 1
    rperm, cperm = rng.permutation(n), rng.permutation(m)
    rows = [[] for _ in range(n)]
    r0 = c0 = 0
    for (a, b) in shapes:
        D = (rng.random((a, b)) < 0.4) * rng.integers(1, p, size=(a, b))
        for i in range(a):  # a path through the rows and columns keeps the block in one component
            D[i, i % b] = D[i, i % b] or 7
            if i + 1 < a:
                D[i + 1, i % b] = D[i + 1, i % b] or 5
        for c in range(b):
            if not D[:, c].any():
                D[c % a, c] = 3
        D[a - 1] = (D[0] * 2) % p
        if not D[a - 1].any():
            D[a - 1, 0] = 1
        for i in range(a):
            rows[rperm[r0 + i]] = [(int(cperm[c0 + c]), int(D[i, c])) for c in range(b) if D[i, c]]
        r0 += a
        c0 += b
    return S.CSR.from_rows(rows, m, prime=p), ncomp


def test_blocks_batched_equals_the_loop(S):
    A, ncomp = block_matrix(S, 200, seed=13)
    B = S.Block.from_csr(A)
    assert len(B) >= ncomp
    want_rank = S.blocks.rank(B, **LM)
    assert S.blocks.rank(B, batched=True, **LM) == want_rank == S.rank(A, **LM)
    st = S.batch_stats()
    assert st["matrices"] == len(B) and st["general_path"] == 0
    want_K = S.blocks.kernel(B, **LM).to_csr()
    got_K = S.blocks.kernel(B, batched=True, **LM).to_csr()
    assert got_K.shape == want_K.shape == (A.m - want_rank, A.m)
    assert sorted(got_K.rows()) == sorted(want_K.rows())
    E = S.blocks.echelonize(B, batched=True, **LM)
    assert S.blocks.rank(E) == want_rank
    assert sorted(S.blocks.kernel(E).to_csr().rows()) == sorted(want_K.rows())
    # owner=(r, 2): each process its share, through one batch call
    shares = []
    for r in range(2):
        loop_rank = S.blocks.rank(B, owner=(r, 2), **LM)
        assert S.blocks.rank(B, owner=(r, 2), batched=True, **LM) == loop_rank
        assert S.batch_stats()["matrices"] == len(range(r, len(B), 2))
        loop_K = S.blocks.kernel(B, owner=(r, 2), **LM).to_csr()
        got = S.blocks.kernel(B, owner=(r, 2), batched=True, **LM).to_csr()
        assert sorted(got.rows()) == sorted(loop_K.rows())
        shares.append((loop_rank, got.rows()))
    assert shares[0][0] + shares[1][0] == want_rank
    assert sorted(shares[0][1] + shares[1][1]) == sorted(want_K.rows())
