"""The resident solver (S.BatchSolver, S.DeviceBlocks.solver) against S.solve_batch / S.DeviceBlocks.solve byte for byte on the LDS
path, and against exact integer arithmetic written here: X * A == B in Python ints mod p, the support of X inside basis(i), and
basis(i) equal to the canonical row basis from a short elimination on the host (row j belongs to it iff it is no combination of rows
0 .. j-1).  Inputs come from seeded numpy generators."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIG = 0xFFFFFFFB
I32 = (-2 ** 31, 2 ** 31 - 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the host side
# ---------------------------------------------------------------------------------------------------------------------------------
def reduce_vec(v, ech, p):
    for lead, e in ech:
        if v[lead]:
            v = (v - v[lead] * e) % p
    return v


def row_basis(D, p):
    """(basis, ech): the canonical row basis of D (entries in [0, p)) and the echelon rows that reduce a vector of its row space to 0"""
    ech, basis = [], []
    for j in range(D.shape[0]):
        v = reduce_vec(D[j].copy(), ech, p)
        nz = np.flatnonzero(v)
        if len(nz):
            v = (v * pow(int(v[nz[0]]), -1, p)) % p
            ech.append((int(nz[0]), v))
            basis.append(j)
    return basis, ech


def dt(p):
    return object if p >= 2 ** 31 else np.int64


def bal(v, p):
    v = int(v) % p
    return v - p if 2 * v > p else v


def csr_of(S, R, stored, p, rng):
    """the CSR that stores R[i, c] (any int32 value) wherever stored[i, c], the entries of a row in random order"""
    n, m = R.shape
    pp, jj, xx = [0], [], []
    for i in range(n):
        cols = np.flatnonzero(stored[i])
        cols = cols[rng.permutation(len(cols))]
        jj += cols.tolist()
        xx += [int(R[i, c]) for c in cols]
        pp.append(len(jj))
    assert all(I32[0] <= v <= I32[1] for v in xx)
    return S.CSR.from_arrays(n, m, np.array(pp, dtype=np.int64), np.array(jj, dtype=np.int32), np.array(xx, dtype=np.int64).astype(np.int32), prime=p)


def dense_csr(S, D, p, rng, zeros=0.05):
    """D (residues in [0, p)) stored balanced, with a few explicit zeros"""
    R = np.array([[bal(v, p) for v in row] for row in D], dtype=object).reshape(D.shape)
    stored = (D != 0) | (rng.random(D.shape) < zeros)
    return csr_of(S, R, stored, p, rng)


def system(rng, n, m, K, p, density=0.5, planted=True):
    """A with duplicated rows, a zero row, a zero column and a row that is a combination of later rows; the even right-hand sides are
    y * A, the odd ones random"""
    A = ((rng.random((n, m)) < density) * rng.integers(1, p, size=(n, m))).astype(dt(p)) % p
    if planted and n >= 6:
        A[0] = (int(rng.integers(1, p)) * A[2] + int(rng.integers(1, p)) * A[n - 1]) % p   # a combination of later rows
        A[3] = A[1]                                                                          # a duplicate
        A[n - 2] = A[1]
        A[n // 2] = 0
    if planted and m >= 3:
        A[:, int(rng.integers(0, m))] = 0
    return A, rhs_for(rng, A, K, p)


def rhs_for(rng, A, K, p):
    n, m = A.shape
    B = np.zeros((K, m), dtype=dt(p))
    for k in range(K):
        if k % 2 == 0 and n:
            y = (rng.integers(0, p, size=n) * (rng.random(n) < 0.6)).astype(dt(p))
            B[k] = (y @ A) % p
        elif k % 5 != 3:
            B[k] = (rng.integers(0, p, size=m) * (rng.random(m) < 0.4)).astype(dt(p)) % p
    return B


def same(Xa, oka, Xb, okb):
    nz = int(Xa.p[Xa.n])
    return (Xa.shape == Xb.shape and Xa.prime == Xb.prime and Xa.nzmax == Xb.nzmax and np.array_equal(Xa.p, Xb.p) and np.array_equal(Xa.j[:nz], Xb.j[:nz])
            and np.array_equal(Xa.x[:nz], Xb.x[:nz]) and oka.dtype == okb.dtype and np.array_equal(oka, okb))


def check_exact(X, ok, A, B, p, basis=None, ech=None):
    """X * A == B in exact integers on the rows with ok, empty rows elsewhere; ok itself and the support when the basis is given"""
    rows = X.rows()
    assert X.shape == (B.shape[0], A.shape[0]) and len(ok) == B.shape[0]
    for k in range(B.shape[0]):
        if ech is not None:
            assert bool(ok[k]) == (not np.any(reduce_vec(B[k].copy() % p, ech, p))), k
        if not ok[k]:
            assert rows[k] == [], k
            continue
        acc = np.zeros(A.shape[1], dtype=dt(p))
        for c, v in rows[k]:
            acc = (acc + (int(v) % p) * A[c]) % p
        assert np.array_equal(acc, B[k] % p), k
        if basis is not None:
            assert set(c for c, _ in rows[k]) <= set(basis), k


def run_lds(S, systems, rng, csrs=None, applies=1):
    """systems: [(A, B, p)] dense; builds the CSRs (or takes them), one solver, compares with solve_batch and the host"""
    mats = [dense_csr(S, A, p, rng) for A, _, p in systems] if csrs is None else csrs[0]
    rhs = [dense_csr(S, B, p, rng) for _, B, p in systems] if csrs is None else csrs[1]
    Xw, okw = S.solve_batch(mats, rhs)
    with S.BatchSolver(mats) as sv:
        assert sv.ranks == S.rank_batch(mats)
        for _ in range(applies):
            X, ok = sv.solve(rhs)
            for i, (A, B, p) in enumerate(systems):
                assert same(X[i], ok[i], Xw[i], okw[i]), i
        info = sv.info()
        for i, (A, B, p) in enumerate(systems):
            basis, ech = row_basis(A, p)
            assert sv.basis(i).tolist() == basis and sv.ranks[i] == len(basis), i
            check_exact(X[i], ok[i], A, B, p, basis, ech)
        assert info["systems"] == len(systems) and info["general_path"] == 0 and info["rank_sum"] == sum(sv.ranks)
    return info


# ---------------------------------------------------------------------------------------------------------------------------------
# the LDS path
# ---------------------------------------------------------------------------------------------------------------------------------
def test_one_system_per_class_full_rank_and_rank_deficient(S):
    rng = np.random.default_rng(1801)
    p = 65521
    systems = []
    for n, m in ((5, 7), (30, 40), (90, 100), (150, 200)):
        systems.append(system(rng, n, m, 6, p, planted=True) + (p,))
        systems.append(system(rng, n, m, 5, p, density=0.7, planted=False) + (p,))
    info = run_lds(S, systems, rng)
    assert info["lds_path"] == 8 and info["factor_jobs"] >= 8
    assert info["operator_words"] == sum(A.shape[1] * len(row_basis(A, p)[0]) for A, _, _ in systems)


def test_mixed_primes_extreme_values_and_unsorted_rows(S):
    rng = np.random.default_rng(1802)
    systems, mats, rhs = [], [], []
    special = [2 ** 31 - 1, -(2 ** 31 - 1), -2 ** 31, 0]
    for p in (3, 127, 65521, BIG):
        n, m, K = 12, 15, 8
        RA = rng.integers(I32[0], I32[1] + 1, size=(n, m))
        RA[rng.random((n, m)) < 0.3] = 0
        RB = rng.integers(I32[0], I32[1] + 1, size=(K, m))
        for R in (RA, RB):
            for v in special:
                R[int(rng.integers(0, R.shape[0])), int(rng.integers(0, R.shape[1]))] = v
        RA[5] = RA[2]
        sa, sb = rng.random((n, m)) < 0.7, rng.random((K, m)) < 0.6
        A = (RA.astype(object) * sa) % p
        for k in range(0, K, 2):   # solvable rows: y * A, stored as balanced residues
            y = rng.integers(0, p, size=n).astype(object)
            RB[k] = np.array([bal(v, p) for v in (y @ A) % p], dtype=object).astype(np.int64)
            sb[k] = True
        B = (RB.astype(object) * sb) % p
        systems.append((A.astype(dt(p)), B.astype(dt(p)), p))
        mats.append(csr_of(S, RA, sa, p, rng))
        rhs.append(csr_of(S, RB, sb, p, rng))
    run_lds(S, systems, rng, csrs=(mats, rhs))


def test_accumulator_bound_180_terms_of_the_largest_product(S):
    rng = np.random.default_rng(1803)
    p, n = BIG, 180
    h = (p - 1) // 2
    A = np.where(rng.random((n, n)) < 0.5, h, p - h).astype(object)
    B = np.where(rng.random((4, n)) < 0.5, h, p - h).astype(object)
    basis, _ = row_basis(A, p)
    assert basis == list(range(n))   # full rank: every right-hand side is solvable, and r = 180 terms meet in every y_i
    info = run_lds(S, [(A, B, p)], rng)
    assert info["operator_words"] == n * n


def test_operator_slabs_when_the_identity_does_not_fit_beside_A(S):
    rng = np.random.default_rng(1804)
    p = 127
    systems = [system(rng, 8, 2000, 4, p, density=0.3) + (p,), system(rng, 16, 1900, 3, p, density=0.3) + (p,)]
    info = run_lds(S, systems, rng)
    assert info["factor_jobs"] > 2 and info["lds_path"] == 2


def test_right_hand_side_slabs_700_against_two_applies_of_350(S):
    rng = np.random.default_rng(1805)
    p = 65521
    A, B = system(rng, 90, 100, 700, p)
    Ac, Bc = dense_csr(S, A, p, rng), dense_csr(S, B, p, rng)
    halves = [S.submatrix(Bc, range(0, 350), range(0, 100)), S.submatrix(Bc, range(350, 700), range(0, 100))]
    (Xw,), (okw,) = S.solve_batch([Ac], [Bc])
    with S.BatchSolver([Ac]) as sv:
        (X,), (ok,) = sv.solve([Bc])
        assert same(X, ok, Xw, okw)
        assert S.solver_stats()["jobs"] > 1
        parts = [sv.solve([H]) for H in halves]
    nz = int(X.p[700])
    assert np.array_equal(np.concatenate([parts[0][1][0], parts[1][1][0]]), ok)
    X0, X1 = parts[0][0][0], parts[1][0][0]
    n0 = int(X0.p[350])
    assert np.array_equal(np.concatenate([X0.p[:351], X1.p[1:351] + n0]), X.p)
    assert np.array_equal(np.concatenate([X0.j[:n0], X1.j[: nz - n0]]), X.j[:nz]) and np.array_equal(np.concatenate([X0.x[:n0], X1.x[: nz - n0]]), X.x[:nz])
    basis, ech = row_basis(A, p)
    check_exact(X, ok, A[:, :], B, p, basis, ech)


def test_edge_shapes(S):
    rng = np.random.default_rng(1806)
    p = 127
    A0, B0 = np.zeros((0, 4), dtype=np.int64), np.array([[0, 3, 0, 0], [0, 0, 0, 0]], dtype=np.int64)     # n = 0
    Am, Bm = np.zeros((3, 0), dtype=np.int64), np.zeros((2, 0), dtype=np.int64)                            # m = 0
    Ak, _ = system(rng, 6, 8, 0, p)                                                                        # K = 0
    Bk = np.zeros((0, 8), dtype=np.int64)
    Ae, Be = system(rng, 6, 8, 5, p)                                                                       # an empty row of B (k = 3)
    assert not Be[3].any()
    Az, Bz = np.zeros((4, 5), dtype=np.int64), np.array([[0, 0, 0, 0, 0], [0, 0, 1, 0, 0]], dtype=np.int64)   # rank 0
    systems = [(A0, B0, p), (Am, Bm, p), (Ak, Bk, p), (Ae, Be, p), (Az, Bz, p)]
    mats = [dense_csr(S, A, p, rng) for A, _, _ in systems]
    mats[4] = csr_of(S, np.full((4, 5), p, dtype=np.int64) * np.arange(-2, 3), np.ones((4, 5), dtype=bool), p, rng)   # stored multiples of p
    rhs = [dense_csr(S, B, p, rng, zeros=0.3) for _, B, _ in systems]
    info = run_lds(S, systems, rng, csrs=(mats, rhs), applies=2)
    assert info["lds_path"] == 5 and info["rank_sum"] == len(row_basis(Ak, p)[0]) + len(row_basis(Ae, p)[0])


def test_reuse_three_applies_and_the_same_input_twice(S):
    rng = np.random.default_rng(1807)
    systems = [system(rng, 20, 24, 4, 65521) + (65521,), system(rng, 9, 30, 4, BIG) + (BIG,), system(rng, 40, 33, 4, 3, density=0.6) + (3,)]
    mats = [dense_csr(S, A, p, rng) for A, _, p in systems]
    with S.BatchSolver(mats) as sv:
        assert sv.ranks == S.rank_batch(mats)
        before = sv.info()
        first = None
        for rep in range(3):
            Bs = [rhs_for(rng, A, 3 + rep, p) for A, _, p in systems]
            rhs = [dense_csr(S, B, q, rng) for B, (_, _, q) in zip(Bs, systems)]
            X, ok = sv.solve(rhs)
            Xw, okw = S.solve_batch(mats, rhs)
            for i, (A, _, p) in enumerate(systems):
                assert same(X[i], ok[i], Xw[i], okw[i]), (rep, i)
                check_exact(X[i], ok[i], A, Bs[i], p, sv.basis(i).tolist())
            if first is None:
                first = (rhs, X, ok)
        X2, ok2 = sv.solve(first[0])
        assert all(same(a, b, c, d) for a, b, c, d in zip(X2, ok2, first[1], first[2]))
        assert sv.info() == before


def test_general_path_among_lds_neighbours(S):
    rng = np.random.default_rng(1808)
    p = 65521
    small = [system(rng, 10, 12, 4, p) + (p,), system(rng, 25, 20, 4, p) + (p,)]
    Ag = ((rng.random((200, 200)) < 0.03) * rng.integers(1, p, size=(200, 200))).astype(np.int64)
    Ag[7] = Ag[3]
    Bg = rhs_for(rng, Ag, 6, p)
    systems = [small[0], (Ag, Bg, p), small[1]]
    mats = [dense_csr(S, A, p, rng, zeros=0) for A, _, p in systems]
    rhs = [dense_csr(S, B, p, rng, zeros=0) for _, B, p in systems]
    Xw, okw = S.solve_batch(mats, rhs)
    with S.BatchSolver(mats) as sv:
        info = sv.info()
        assert (info["systems"], info["lds_path"], info["general_path"]) == (3, 2, 1)
        for _ in range(2):
            X, ok = sv.solve(rhs)
            assert same(X[0], ok[0], Xw[0], okw[0]) and same(X[2], ok[2], Xw[2], okw[2])
            assert np.array_equal(ok[1], okw[1])
            _, ech = row_basis(Ag, p)
            check_exact(X[1], ok[1], Ag, Bg, p, sv.basis(1).tolist(), ech)
        assert len(sv.basis(1)) == sv.ranks[1] == len(ech)
        st = S.solver_stats()
        assert (st["systems"], st["lds_path"], st["general_path"]) == (3, 2, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# block by block
# ---------------------------------------------------------------------------------------------------------------------------------
def block_matrix(rng, p, big):
    """about 40 components of mixed small shapes (and one over the limit when `big`) on the diagonal, an empty row and an empty
    column, under a random row and column permutation; the last column is the empty one after the permutation is undone"""
    shapes = [(int(rng.integers(1, 6)), int(rng.integers(1, 7))) for _ in range(40)] + ([(200, 200)] if big else [])
    n, m = sum(a for a, _ in shapes) + 1, sum(b for _, b in shapes) + 1
    A = np.zeros((n, m), dtype=np.int64)
    r0 = c0 = 0
    for a, b in shapes:
        blk = rng.integers(1, p, size=(a, b)) * (rng.random((a, b)) < (0.03 if a == 200 else 0.8))
        blk[0, :] = rng.integers(1, p, size=b) if a < 200 else blk[0, :]
        blk[:, 0] = np.maximum(blk[:, 0], 1) if a < 200 else blk[:, 0]   # connected: the first row and the first column are full
        A[r0:r0 + a, c0:c0 + b] = blk
        r0, c0 = r0 + a, c0 + b
    rp, cp = rng.permutation(n), rng.permutation(m)
    A = A[rp][:, cp]
    return A, int(np.flatnonzero(cp == m - 1)[0])


def test_blocks_solver_equals_blocks_solve_and_solve_batch(S):
    rng = np.random.default_rng(1809)
    p = 127
    A, empty_col = block_matrix(rng, p, big=False)
    n, m = A.shape
    assert m * (n + 1) <= 32768 and not A[:, empty_col].any()
    B = rhs_for(rng, A, 12, p)
    B[4, empty_col] = 5                 # a solvable row made unsolvable by the empty column
    Ac, Bc = dense_csr(S, A, p, rng), dense_csr(S, B, p, rng)
    with S.DeviceBlocks(Ac) as db:
        Xd, okd = db.solve(Bc)
        sv = db.solver()
        X, ok = sv.solve(Bc)
        assert same(X, ok, Xd, okd)
    # the DeviceBlocks is closed; the solver holds its own maps
    with sv:
        X2, ok2 = sv.solve(Bc)
        assert same(X2, ok2, Xd, okd)
        (Xw,), (okw,) = S.solve_batch([Ac], [Bc])
        assert same(X2, ok2, Xw, okw)
        assert not ok2[4] and ok2[0] and ok2[2]
        basis, ech = row_basis(A, p)
        check_exact(X2, ok2, A, B, p, basis, ech)
        info = sv.info()
        assert info["general_path"] == 0 and info["rank_sum"] == len(basis) and info["systems"] == len(sv)
        # errors on a live handle: the outputs stay as they were and the handle stays usable
        out = (C.POINTER(S._abi.CsrStruct) * 1)()
        raw = C.cast(out, C.POINTER(C.c_uint64))
        raw[0] = 0x5A5A5A5A
        okb = np.full(12, 0xA5, dtype=np.uint8)
        okp = okb.ctypes.data_as(C.POINTER(C.c_ubyte))
        lib, err = S._abi.lib(), S._abi.last_error
        wrong_m = S.CSR.from_rows([[(0, 1)]], m + 1, prime=p)
        wrong_p = S.CSR.from_rows([[(0, 1)]], m, prime=65521)
        assert lib.spasm_amd_solver_apply_blocks(sv._need(), wrong_m.data, out, okp) == -1 and err().startswith("spasm_amd_solver_apply_blocks") and "Rhs->m" in err()
        assert lib.spasm_amd_solver_apply_blocks(sv._need(), wrong_p.data, out, okp) == -1 and "prime" in err()
        brr = (C.POINTER(S._abi.CsrStruct) * 1)(Bc.data)
        okpp = (C.POINTER(C.c_ubyte) * 1)(okp)
        assert lib.spasm_amd_solver_apply(sv._need(), brr, out, okpp) == -1 and err().startswith("spasm_amd_solver_apply:") and "create_blocks" in err()
        assert raw[0] == 0x5A5A5A5A and (okb == 0xA5).all()
        X3, ok3 = sv.solve(Bc)
        assert same(X3, ok3, Xd, okd)


def test_blocks_solver_with_a_block_over_the_limit(S):
    rng = np.random.default_rng(1810)
    p = 127
    A, empty_col = block_matrix(rng, p, big=True)
    B = rhs_for(rng, A, 8, p)
    B[2, empty_col] = 9
    Ac, Bc = dense_csr(S, A, p, rng, zeros=0), dense_csr(S, B, p, rng, zeros=0)
    with S.DeviceBlocks(Ac) as db:
        Xd, okd = db.solve(Bc)
        with db.solver() as sv:
            assert sv.info()["general_path"] == 1
            for _ in range(2):
                X, ok = sv.solve(Bc)
                assert np.array_equal(ok, okd) and not ok[2]
                _, ech = row_basis(A, p)
                check_exact(X, ok, A, B, p, None, ech)
            assert sum(sv.ranks) == len(ech)


def test_errors_on_a_live_list_handle(S):
    rng = np.random.default_rng(1811)
    p = 127
    A, B = system(rng, 7, 9, 3, p)
    Ac, Bc = dense_csr(S, A, p, rng), dense_csr(S, B, p, rng)
    with S.BatchSolver([Ac, Ac]) as sv:
        want = sv.solve([Bc, Bc])
        lib, err = S._abi.lib(), S._abi.last_error
        out = (C.POINTER(S._abi.CsrStruct) * 2)()
        raw = C.cast(out, C.POINTER(C.c_uint64))
        raw[0] = raw[1] = 0x5A5A5A5A
        oks = [np.full(3, 0xA5, dtype=np.uint8) for _ in range(2)]
        okp = (C.POINTER(C.c_ubyte) * 2)(*[o.ctypes.data_as(C.POINTER(C.c_ubyte)) for o in oks])

        def apply(b0, b1):
            return lib.spasm_amd_solver_apply(sv._need(), (C.POINTER(S._abi.CsrStruct) * 2)(b0.data, b1.data), out, okp)

        assert apply(Bc, S.CSR.from_rows([[], [], []], 10, prime=p)) == -1 and err().startswith("spasm_amd_solver_apply:") and "matrix 1" in err() and "B->m != A->m" in err()
        assert apply(S.CSR.from_rows([[], [], []], 9, prime=3), Bc) == -1 and "matrix 0" in err() and "primes" in err()
        assert lib.spasm_amd_solver_apply_blocks(sv._need(), Bc.data, out, okp[0]) == -1 and err().startswith("spasm_amd_solver_apply_blocks")
        assert raw[0] == 0x5A5A5A5A and raw[1] == 0x5A5A5A5A and all((o == 0xA5).all() for o in oks)
        got = sv.solve([Bc, Bc])
        assert all(same(a, b, c, d) for a, b, c, d in zip(got[0], got[1], want[0], want[1]))
