"""The dense apply of the resident solver (S.BatchSolver.solve_dense) on torch tensors that stay on the device, against two
yardsticks: (a) S.BatchSolver.solve on the same right-hand sides as CSR, densified, entry for entry (np.array_equal, no tolerance);
(b) exact integer arithmetic written here: X[:, v] * A == B[:, v] in Python / int64 integers mod p for every column with ok, X zero
outside basis(i), balanced residues, and an all-zero column where ok is False.  Every test plants solvable right-hand sides (y * A)
and unsolvable ones (random against a rank-deficient A) and asserts that both kinds occurred.  Inputs come from seeded generators;
the helpers are those of test_gpu_solver.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIG = 0xFFFFFFFB
I32 = (-2 ** 31, 2 ** 31 - 1)
T = 8           # SOLVER_DENSE_T: the register tile of k_solver_apply_dense
SENTINEL = 0x5A5A5A5A


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


def balanced(D, p):
    return np.array([[bal(v, p) for v in row] for row in D], dtype=np.int64).reshape(D.shape)


def system(rng, n, m, K, p, density=0.5, planted=True):
    """A with duplicated rows, a zero row, a zero column and a row that is a combination of later rows; the even right-hand sides are
    y * A, the odd ones random"""
    A = ((rng.random((n, m)) < density) * rng.integers(1, p, size=(n, m))).astype(dt(p)) % p
    if planted and n >= 6:
        A[0] = (int(rng.integers(1, p)) * A[2] + int(rng.integers(1, p)) * A[n - 1]) % p
        A[3] = A[1]
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


def densify(Xc):
    """the K x n CSR of solve as the n x K array of solve_dense"""
    K, n = Xc.shape
    D = np.zeros((n, K), dtype=np.int64)
    for k in range(K):
        e0, e1 = int(Xc.p[k]), int(Xc.p[k + 1])
        D[np.asarray(Xc.j[e0:e1]), k] = np.asarray(Xc.x[e0:e1])
    return D


def check_exact(X, ok, A, R, p, basis, ech=None):
    """X (n x K), ok (K) against A (n x m, residues) and the raw right-hand sides R (K x m, any integers), in exact integers"""
    n, K = X.shape
    Ao = A.astype(object)
    out = np.setdiff1d(np.arange(n), np.asarray(basis, dtype=np.int64))
    assert np.all(np.abs(X) <= p // 2)
    for v in range(K):
        if ech is not None:
            assert bool(ok[v]) == (not np.any(reduce_vec(np.array([int(x) % p for x in R[v]], dtype=dt(p)), ech, p))), v
        if not ok[v]:
            assert not X[:, v].any(), v
            continue
        got = X[:, v].astype(object) @ Ao if n else np.zeros(A.shape[1], dtype=object)
        assert all((int(g) - int(b)) % p == 0 for g, b in zip(got, R[v])), v
        assert not X[out, v].any(), v


def to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_list(S, systems, rng, raw=None, check_ok=True):
    """systems: [(A, B, p)], A dense residues, B (K x m) residues, the same K everywhere; raw[i]: the int32 values of B[i] as stored.
    One list solver: solve on CSR, solve_dense on a device tensor, both yardsticks.  Returns (X, ok, solver info, kinds seen)."""
    mats = [csr_of(S, balanced(A, p), (A != 0) | (rng.random(A.shape) < 0.05), p, rng) for A, _, p in systems]
    raw = [balanced(B, p) for _, B, p in systems] if raw is None else raw
    rhs = [csr_of(S, R, R != 0, p, rng) for R, (_, _, p) in zip(raw, systems)]
    K = raw[0].shape[0]
    Bd = np.concatenate([R.T for R in raw], axis=0).astype(np.int32)
    with S.BatchSolver(mats) as sv:
        Xs, oks = sv.solve(rhs)
        Bt = to_dev(Bd)
        X, ok = sv.solve_dense(Bt)
        assert tuple(X.shape) == (sum(A.shape[0] for A, _, _ in systems), K) and tuple(ok.shape) == (len(systems), K)
        Xh, okh = X.cpu().numpy().astype(np.int64), ok.cpu().numpy()
        assert np.array_equal(Bt.cpu().numpy(), Bd)                      # B is left as it was
        r0 = 0
        for i, (A, _, p) in enumerate(systems):
            n = A.shape[0]
            assert np.array_equal(Xh[r0:r0 + n], densify(Xs[i])), i      # (a)
            assert np.array_equal(okh[i], oks[i]), i
            basis, ech = row_basis(A, p) if check_ok else (sv.basis(i).tolist(), None)
            assert sv.basis(i).tolist() == basis and sv.ranks[i] == len(basis), i
            check_exact(Xh[r0:r0 + n], okh[i], A, raw[i], p, basis, ech)   # (b)
            r0 += n
        info = sv.dense_info()
        ranks = sv.ranks
    assert okh.any() and not okh.all()                                   # both kinds occurred
    return Xh, okh, info, ranks


# ---------------------------------------------------------------------------------------------------------------------------------
# a list of systems
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [127, 65521])
def test_image_rows_across_the_wave_and_group_boundaries(S, p):
    """m = 1, 63, 64, 65 (one wave, and one row more), 50 (two groups in a workgroup of 128) and 600 (above every workgroup: the
    rows stride)"""
    rng = np.random.default_rng(1901)
    systems = []
    for n, m in ((1, 1), (3, 63), (3, 64), (3, 65), (40, 50), (1, 600)):
        systems.append(system(rng, n, m, 5, p, density=0.6, planted=n >= 6) + (p,))
    systems[0][0][0, 0] = 3
    _, ok, info, ranks = run_list(S, systems, rng)
    assert ranks[0] == 1 and ranks[5] == 1 and ranks[4] < 40
    assert (info["rows"], info["cols"], info["ok_rows"], info["plan_k"], info["plan_jobs"]) == (51, 843, 6, 5, 6)


def test_rank_zero_odd_and_even_rank_and_every_class(S):
    rng = np.random.default_rng(1902)
    p = 65521
    K = 6
    Az = np.zeros((4, 5), dtype=np.int64)                      # rank 0: ok iff the right-hand side vanishes
    Bz = np.zeros((K, 5), dtype=np.int64)
    Bz[1, 2] = 1
    Bz[4] = rng.integers(1, p, size=5)
    systems = [(Az, Bz, p)]
    for n in (5, 6):                                           # full rank 5 (ldg = r) and 6 (ldg = r + 1)
        A = rng.integers(1, p, size=(n, 9)).astype(np.int64)
        systems.append((A, rhs_for(rng, A, K, p), p))
    for n, m in ((5, 7), (30, 40), (90, 100), (150, 200)):     # one full-rank and one rank-deficient system in every class
        systems.append(system(rng, n, m, K, p, planted=True) + (p,))
        systems.append(system(rng, n, m, K, p, density=0.7, planted=False) + (p,))
    _, ok, info, ranks = run_list(S, systems, rng)
    assert ranks[:3] == [0, 5, 6]
    assert ok[0].tolist() == [True, False, True, True, False, True]
    assert ranks[4] == 5 and ranks[6] == 30 and ranks[8] == 90 and ranks[10] == 150
    assert ranks[5] < 30 and ranks[7] < 90 and ranks[9] < 150
    assert info["plan_launches"] == 4                          # four classes, one launch each, and nothing else


def test_columns_against_the_tile_and_the_slab(S):
    """K = 1, 2, T - 1, T, T + 1, and K = 300: more than a slab of either system (64 columns for the first, 128 for the second), so a
    system takes several workgroups.  Where the slabs are cut does not matter: the halves, as views of the same tensor (ldb > K),
    give the columns of the whole."""
    rng = np.random.default_rng(1903)
    p = 65521
    pair = [system(rng, 5, 7, 300, p) + (p,), system(rng, 40, 50, 300, p) + (p,)]
    seen = {}
    for K in (2, T - 1, T, T + 1, 300):                        # (K = 1 cannot hold both kinds: it is the vector further down)
        systems = [(A, B[:K], q) for A, B, q in pair]
        X, ok, info, _ = run_list(S, systems, rng)
        seen[K] = (X, ok)
        if K == 300:
            assert info["plan_jobs"] == 5 + 3
    X, ok = seen[300]
    for K in (2, T - 1, T, T + 1):
        assert np.array_equal(seen[K][0], X[:, :K]) and np.array_equal(seen[K][1], ok[:, :K])
    raw = [balanced(B, q) for _, B, q in pair]
    mats = [csr_of(S, balanced(A, q), A != 0, q, rng) for A, _, q in pair]
    Bt = to_dev(np.concatenate([R.T for R in raw], axis=0).astype(np.int32))
    with S.BatchSolver(mats) as sv:
        (X0, ok0), (X1, ok1) = sv.solve_dense(Bt[:, :150]), sv.solve_dense(Bt[:, 150:])
        for v in (3, 0, 1):                                    # a vector: shape (M,), K = 1: the zero vector, a solvable one and one without solution
            one = sv.solve_dense(Bt[:, v].contiguous())
            assert tuple(one[0].shape) == (45,) and tuple(one[1].shape) == (2,)
            assert np.array_equal(one[0].cpu().numpy(), X[:, v]) and np.array_equal(one[1].cpu().numpy(), ok[:, v])
        assert ok[:, 3].all() and not X[:, 3].any() and ok[:, 0].all() and X[:5, 0].any() and X[5:, 0].any() and not ok[:, 1].any()
    assert np.array_equal(np.concatenate([X0.cpu().numpy(), X1.cpu().numpy()], axis=1), X)
    assert np.array_equal(np.concatenate([ok0.cpu().numpy(), ok1.cpu().numpy()], axis=1), ok)


def test_leading_dimensions_leave_the_words_outside_the_windows(S):
    import torch

    rng = np.random.default_rng(1904)
    p = 127
    K = 11
    systems = [system(rng, 7, 9, K, p) + (p,), system(rng, 12, 10, K, p) + (p,)]
    Xw, okw, _, _ = run_list(S, systems, rng)
    raw = [balanced(B, q) for _, B, q in systems]
    mats = [csr_of(S, balanced(A, q), A != 0, q, rng) for A, _, q in systems]
    Bd = np.concatenate([R.T for R in raw], axis=0).astype(np.int32)
    M, N = Bd.shape[0], 19
    with S.BatchSolver(mats) as sv:
        # the device: windows inside sentinel-filled tensors
        Bbig = torch.full((M, K + 5), 77, dtype=torch.int32, device="cuda")
        Xbig = torch.full((N, K + 3), SENTINEL, dtype=torch.int32, device="cuda")
        Bbig[:, 2:2 + K] = to_dev(Bd)
        keep = Bbig.clone()
        X, ok = sv.solve_dense(Bbig[:, 2:2 + K], X=Xbig[:, 1:1 + K])
        assert X.data_ptr() == Xbig[:, 1:1 + K].data_ptr()
        assert torch.equal(Bbig, keep)
        Xb = Xbig.cpu().numpy()
        assert (Xb[:, 0] == SENTINEL).all() and (Xb[:, 1 + K:] == SENTINEL).all()
        assert np.array_equal(Xb[:, 1:1 + K], Xw) and np.array_equal(ok.cpu().numpy(), okw)
        # the host entry: the same windows in numpy arrays
        Bh = np.full((M, K + 5), 77, dtype=np.int32)
        Bh[:, 2:2 + K] = Bd
        keeph = Bh.copy()
        Xh = np.full((N, K + 3), SENTINEL, dtype=np.int32)
        Xv, okv = sv.solve_dense(Bh[:, 2:2 + K], X=Xh[:, 1:1 + K])
        assert np.array_equal(Bh, keeph) and (Xh[:, 0] == SENTINEL).all() and (Xh[:, 1 + K:] == SENTINEL).all()
        assert np.array_equal(Xh[:, 1:1 + K], Xw) and np.array_equal(okv, okw) and okv.dtype == np.bool_
    for i, r0, n in ((0, 0, 7), (1, 7, 12)):
        assert not Xw[r0:r0 + n][:, ~okw[i]].any()            # a column without solution is all zero


def test_any_int32_is_reduced_on_load_with_mixed_primes(S):
    rng = np.random.default_rng(1905)
    systems, raw = [], []
    n, m, K = 12, 15, 8
    for p in (127, 65521, BIG):
        A = ((rng.random((n, m)) < 0.7) * rng.integers(1, p, size=(n, m))).astype(dt(p)) % p
        A[5] = A[2]
        A[9] = 0
        R = rng.integers(I32[0], I32[1] + 1, size=(K, m))
        for k in range(0, K, 2):                               # solvable: y * A as balanced residues, then shifted by multiples of p
            y = rng.integers(0, p, size=n).astype(dt(p))
            R[k] = balanced(((y @ A) % p).reshape(1, m), p)[0]
        special = [I32[0], I32[1]] + ([p, -p, 2 * p, -3 * p] if p < 2 ** 31 else [])
        for k in (1, 3):                                       # unsolvable rows keep the extreme values as they are
            for v in special:
                R[k, int(rng.integers(0, m))] = v
        if p < 2 ** 31:                                        # a solvable row stays solvable under + p, - p on its entries
            R[0, 0] += p
            R[0, 1] -= p
            R[2, 3] = R[2, 3] + (2 ** 31 - 1 - R[2, 3]) // p * p     # the largest int32 in its residue class
            R[2, 4] = R[2, 4] - (R[2, 4] + 2 ** 31) // p * p         # the smallest
        systems.append((A, R % p if p < 2 ** 31 else np.array([[int(v) % p for v in row] for row in R], dtype=object), p))
        raw.append(R.astype(np.int64))
    _, ok, _, _ = run_list(S, systems, rng, raw=raw)
    assert ok[:, 0::2].all()


@pytest.mark.parametrize("p", [BIG, 65521])
def test_accumulator_bound_180_terms_of_the_largest_product(S, p):
    """r = 180 terms of +-((p - 1) / 2)^2 meet in every y_i of the full-rank system; its rank-deficient neighbour (duplicated rows,
    m - r >= 31) supplies the right-hand sides without solution"""
    rng = np.random.default_rng(1906)
    n = 180
    h = (p - 1) // 2
    A = np.where(rng.random((n, n)) < 0.5, h, p - h).astype(dt(p))
    B = np.where(rng.random((4, n)) < 0.5, h, p - h).astype(dt(p))
    A2 = np.where(rng.random((60, 90)) < 0.5, h, p - h).astype(dt(p))
    A2[7] = A2[3]
    B2 = np.where(rng.random((4, 90)) < 0.5, h, p - h).astype(dt(p))
    B2[2] = (np.where(rng.random(60) < 0.5, h, p - h).astype(dt(p)) @ A2) % p
    _, ok, _, ranks = run_list(S, [(A, B, p), (A2, B2, p)], rng, check_ok=p < 2 ** 31)
    assert ranks[0] == n and ranks[1] < 60
    assert ok[0].all() and ok[1].tolist() == [False, False, True, False]


def test_plan_cache_reuse_and_the_sparse_apply_afterwards(S):
    rng = np.random.default_rng(1907)
    p = 65521
    systems = [system(rng, 20, 24, 9, p) + (p,), system(rng, 9, 30, 9, p) + (p,)]
    raw = [balanced(B, q) for _, B, q in systems]
    mats = [csr_of(S, balanced(A, q), A != 0, q, rng) for A, _, q in systems]
    rhs = [csr_of(S, R, R != 0, q, rng) for R, (_, _, q) in zip(raw, systems)]
    Bt = to_dev(np.concatenate([R.T for R in raw], axis=0).astype(np.int32))
    with S.BatchSolver(mats) as sv:
        before = sv.solve(rhs)
        assert sv.dense_info()["plans_built"] == 0 and sv.dense_info()["plan_k"] == 0
        X1, ok1 = sv.solve_dense(Bt[:, :5].contiguous())
        i1 = sv.dense_info()
        X2, ok2 = sv.solve_dense(Bt[:, :5].contiguous())
        assert sv.dense_info() == i1 and (i1["plan_k"], i1["plans_built"], i1["plan_jobs"], i1["plan_launches"]) == (5, 1, 2, 1)
        X3, ok3 = sv.solve_dense(Bt)
        i3 = sv.dense_info()
        assert (i3["plan_k"], i3["plans_built"]) == (9, 2)
        assert np.array_equal(X1.cpu().numpy(), X2.cpu().numpy()) and np.array_equal(ok1.cpu().numpy(), ok2.cpu().numpy())
        assert np.array_equal(X3.cpu().numpy()[:, :5], X1.cpu().numpy()) and np.array_equal(ok3.cpu().numpy()[:, :5], ok1.cpu().numpy())
        ok3 = ok3.cpu().numpy()
        assert ok3.any() and not ok3.all()
        r0 = 0
        for i in range(2):
            n = systems[i][0].shape[0]
            assert np.array_equal(X3.cpu().numpy()[r0:r0 + n], densify(before[0][i])) and np.array_equal(ok3[i], before[1][i])
            r0 += n
        after = sv.solve(rhs)
        for i in range(2):
            assert np.array_equal(densify(after[0][i]), densify(before[0][i])) and np.array_equal(after[1][i], before[1][i])
            assert np.array_equal(after[0][i].p, before[0][i].p)


def test_a_system_over_the_limit_is_refused_and_named(S):
    import torch

    rng = np.random.default_rng(1908)
    p = 65521
    small = [system(rng, 10, 12, 4, p) + (p,), system(rng, 25, 20, 4, p) + (p,)]
    Ag = ((rng.random((200, 200)) < 0.03) * rng.integers(1, p, size=(200, 200))).astype(np.int64)
    systems = [small[0], (Ag, rhs_for(rng, Ag, 4, p), p), small[1]]
    mats = [csr_of(S, balanced(A, q), A != 0, q, rng) for A, _, q in systems]
    rhs = [csr_of(S, balanced(B, q), B != 0, q, rng) for _, B, q in systems]
    with S.BatchSolver(mats) as sv:
        want = sv.solve(rhs)
        assert sv.dense_info()["general_path"] == 1 and sv.dense_info()["rows"] == 235 and sv.dense_info()["cols"] == 232
        Bt = torch.ones((232, 4), dtype=torch.int32, device="cuda")
        Xt = torch.full((235, 4), SENTINEL, dtype=torch.int32, device="cuda")
        okt = torch.full((12,), 0xA5, dtype=torch.uint8, device="cuda")
        with pytest.raises(S.SpasmError, match="spasm_amd_solver_apply_dense_dev: system 1 "):
            sv.solve_dense(Bt, X=Xt)
        rc = S._abi.lib().spasm_amd_solver_apply_dense_dev(sv._need(), 4, C.c_void_p(Bt.data_ptr()), 4, C.c_void_p(Xt.data_ptr()), 4, C.c_void_p(okt.data_ptr()), None)
        assert rc == -1 and "system 1 " in S._abi.last_error() and "general path" in S._abi.last_error()
        with pytest.raises(S.SpasmError, match="spasm_amd_solver_apply_dense: system 1 "):
            sv.solve_dense(np.ones((232, 4), dtype=np.int32))
        assert bool((Xt == SENTINEL).all()) and bool((okt == 0xA5).all()) and bool((Bt == 1).all())
        assert sv.dense_info()["plans_built"] == 0
        got = sv.solve(rhs)
        for i in range(3):
            assert np.array_equal(densify(got[0][i]), densify(want[0][i])) and np.array_equal(got[1][i], want[1][i])
    # the right-hand sides of the two small systems, on a solver of their own, are of both kinds (the refusal itself solves nothing)
    _, ok, _, _ = run_list(S, small, rng)


# ---------------------------------------------------------------------------------------------------------------------------------
# the blocks of a split matrix
# ---------------------------------------------------------------------------------------------------------------------------------
def block_matrix(rng, p):
    """about 40 components of mixed small shapes, a 1 x 1 block among them, on the diagonal, an empty row and an empty column, under
    a random row and column permutation (the rows and columns of the blocks interleave); returns A, the empty column, the empty row"""
    shapes = [(int(rng.integers(1, 6)), int(rng.integers(1, 7))) for _ in range(39)] + [(1, 1)]
    n, m = sum(a for a, _ in shapes) + 1, sum(b for _, b in shapes) + 1
    A = np.zeros((n, m), dtype=np.int64)
    r0 = c0 = 0
    for a, b in shapes:
        blk = rng.integers(1, p, size=(a, b)) * (rng.random((a, b)) < 0.8)
        blk[0, :] = rng.integers(1, p, size=b)
        blk[:, 0] = np.maximum(blk[:, 0], 1)   # connected: the first row and the first column are full
        A[r0:r0 + a, c0:c0 + b] = blk
        r0, c0 = r0 + a, c0 + b
    rp, cp = rng.permutation(n), rng.permutation(m)
    A = A[rp][:, cp]
    return A, int(np.flatnonzero(cp == m - 1)[0]), int(np.flatnonzero(rp == n - 1)[0])


def test_blocks_solver_dense_equals_blocks_solve_and_solve_batch(S):
    import torch

    rng = np.random.default_rng(1909)
    p = 127
    A, empty_col, empty_row = block_matrix(rng, p)
    n, m = A.shape
    assert m * (n + 1) <= 32768 and not A[:, empty_col].any() and not A[empty_row].any()
    K = 12
    B = rhs_for(rng, A, K, p)
    assert not B[4, empty_col] and not B[6, empty_col]
    raw = balanced(B, p)
    raw[4, empty_col] = 5                   # a solvable right-hand side made unsolvable by the empty column, and by nothing else
    raw[6, empty_col] = 3 * p               # ... while a multiple of p there changes nothing
    Ac = csr_of(S, balanced(A, p), (A != 0) | (rng.random(A.shape) < 0.05), p, rng)
    Bc = csr_of(S, raw, raw != 0, p, rng)
    Bt = to_dev(raw.T.astype(np.int32))
    with S.DeviceBlocks(Ac) as db:
        Xd, okd = db.solve(Bc)
        sv = db.solver()
    with sv:                                # the DeviceBlocks is closed; the solver holds its own maps
        # X is a window of a sentinel-filled tensor (ldx > K): every word of the window has to be stored, the rows of the empty
        # row of A, of the blocks without rank and outside the basis included, and no word beside it
        Xbig = torch.full((n, K + 3), SENTINEL, dtype=torch.int32, device="cuda")
        X, ok = sv.solve_dense(Bt, X=Xbig[:, 2:2 + K])
        assert tuple(X.shape) == (n, K) and tuple(ok.shape) == (K,) and X.data_ptr() == Xbig[:, 2:2 + K].data_ptr()
        Xb = Xbig.cpu().numpy()
        assert (Xb[:, :2] == SENTINEL).all() and (Xb[:, 2 + K:] == SENTINEL).all()
        Xh, okh = X.cpu().numpy().astype(np.int64), ok.cpu().numpy()
        assert np.array_equal(Xh, densify(Xd)) and np.array_equal(okh, okd)
        (Xw,), (okw,) = S.solve_batch([Ac], [Bc])
        assert np.array_equal(Xh, densify(Xw)) and np.array_equal(okh, okw)
        Xs, oks = sv.solve(Bc)
        assert np.array_equal(Xh, densify(Xs)) and np.array_equal(okh, oks)
        basis, ech = row_basis(A, p)
        check_exact(Xh, okh, A, raw, p, basis, ech)
        assert not okh[4] and okh[0] and okh[2] and okh[6] and not okh.all()
        assert not Xh[empty_row].any()
        info = sv.dense_info()
        assert (info["rows"], info["cols"], info["ok_rows"], info["general_path"], info["plan_k"]) == (n, m, 1, 0, K)
        assert info["plan_jobs"] == len(sv)
        # without the entry on the empty column that column, and only that column, turns solvable
        Bt[empty_col, 4] = 0
        X2, ok2 = sv.solve_dense(Bt)
        ok2 = ok2.cpu().numpy()
        assert ok2[4] and np.array_equal(np.delete(ok2, 4), np.delete(okh, 4))
        assert np.array_equal(np.delete(X2.cpu().numpy(), 4, axis=1), np.delete(Xh, 4, axis=1)) and X2.cpu().numpy()[:, 4].any()
        # the host entry
        Xn, okn = sv.solve_dense(np.ascontiguousarray(raw.T.astype(np.int32)))
        assert np.array_equal(Xn, Xh) and np.array_equal(okn, okh)


def test_solve_residual_and_solve_again_on_one_stream(S):
    """X, ok = solve_dense(B); R = B - A^T X through the resident product; solve_dense(R): all on one non-default stream, one
    synchronise at the end, and no right-hand side on the host in between"""
    import torch

    rng = np.random.default_rng(1910)
    p = 65521
    K = 10
    A, B = system(rng, 40, 50, K, p)
    Ac = csr_of(S, balanced(A, p), A != 0, p, rng)
    Bt = to_dev(balanced(B, p).T.astype(np.int32))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with S.BatchSolver([Ac]) as sv, S.SpMV(Ac) as op:
        with torch.cuda.stream(stream):
            X, ok = sv.solve_dense(Bt)
            R = Bt.clone()
            op.apply(-X, R, trans=True)          # R <- A^T (-X) + R, column by column: b - x A
            X2, ok2 = sv.solve_dense(R)
        stream.synchronize()
        Xh, okh, Rh = X.cpu().numpy().astype(np.int64), ok.cpu().numpy()[0], R.cpu().numpy().astype(np.int64)
        assert okh.any() and not okh.all()
        assert not (Rh[:, okh] % p).any()
        assert np.array_equal(Rh[:, ~okh] % p, (balanced(B, p).T % p)[:, ~okh])      # where nothing was solved, R is still B
        assert np.array_equal(ok2.cpu().numpy()[0], okh) and not X2.cpu().numpy().any()
        basis, ech = row_basis(A, p)
        check_exact(Xh, okh, A, balanced(B, p), p, basis, ech)
        (Xs,), (oks,) = sv.solve([csr_of(S, balanced(B, p), B != 0, p, rng)])
        assert np.array_equal(Xh, densify(Xs)) and np.array_equal(okh, oks)


def test_two_plans_back_to_back_on_a_busy_stream(S):
    """Applies of K = 9, 5 and 9 again follow each other on a non-default stream that is still busy with earlier work, without a
    synchronise in between: the plan of a new K must not replace the plan an apply enqueued earlier has yet to read (the number
    of jobs is the same for both K, so the buffers of the plan are reused).  Every X is a window of a sentinel-filled tensor wide
    enough for either K.  Afterwards K = 0 on a handle with a system of the general path succeeds, and B and X that overlap in
    part are refused in Python."""
    import torch

    rng = np.random.default_rng(1911)
    p = 65521
    systems = [system(rng, 20, 24, 9, p) + (p,), system(rng, 9, 30, 9, p) + (p,)]
    raw = [balanced(B, q) for _, B, q in systems]
    mats = [csr_of(S, balanced(A, q), A != 0, q, rng) for A, _, q in systems]
    rhs = [csr_of(S, R, R != 0, q, rng) for R, (_, _, q) in zip(raw, systems)]
    Bd = np.concatenate([R.T for R in raw], axis=0).astype(np.int32)
    N, W = 29, 16
    with S.BatchSolver(mats) as sv:
        Xs, oks = sv.solve(rhs)
        want = np.concatenate([densify(x) for x in Xs], axis=0)
        wok = np.stack(oks)
        assert wok[:, :5].any() and not wok[:, :5].all()        # both kinds occur, among the first five columns already
        B9, B5, B9b = to_dev(Bd), to_dev(Bd[:, :5]), to_dev(Bd[:, ::-1])
        big = [torch.full((N, W), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
        load = torch.zeros(1 << 26, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            for _ in range(16):                  # a few milliseconds of work ahead of the first apply
                load.add_(1)
            _, ok9 = sv.solve_dense(B9, X=big[0][:, 1:10])
            _, ok5 = sv.solve_dense(B5, X=big[1][:, 1:6])
            _, ok9b = sv.solve_dense(B9b, X=big[2][:, 1:10])
        stream.synchronize()
        assert sv.dense_info()["plans_built"] == 3 and sv.dense_info()["plan_jobs"] == 2
        assert int(load[0]) == 16
        for Xw, ok, K, Xwant, okwant in ((big[0], ok9, 9, want, wok), (big[1], ok5, 5, want[:, :5], wok[:, :5]), (big[2], ok9b, 9, want[:, ::-1], wok[:, ::-1])):
            Xw = Xw.cpu().numpy()
            assert np.array_equal(Xw[:, 1:1 + K], Xwant) and np.array_equal(ok.cpu().numpy(), okwant), K
            assert (Xw[:, 0] == SENTINEL).all() and (Xw[:, 1 + K:] == SENTINEL).all(), K
        # B and X that overlap in part (not at their first word) are refused before the engine is called
        both = torch.zeros((54 + N, 9), dtype=torch.int32, device="cuda")
        with pytest.raises(ValueError, match="overlap"):
            sv.solve_dense(both[:54], X=both[54 - 3:54 - 3 + N])
        assert sv.dense_info()["plans_built"] == 3
    # K = 0 has nothing to refuse, on a handle with a system of the general path too
    Ag = ((rng.random((200, 200)) < 0.03) * rng.integers(1, p, size=(200, 200))).astype(np.int64)
    with S.BatchSolver([mats[0], csr_of(S, balanced(Ag, p), Ag != 0, p, rng)]) as sv:
        assert sv.dense_info()["general_path"] == 1
        X0, ok0 = sv.solve_dense(torch.zeros((224, 0), dtype=torch.int32, device="cuda"))
        assert tuple(X0.shape) == (220, 0) and tuple(ok0.shape) == (2, 0)
        with pytest.raises(S.SpasmError, match="system 1 "):
            sv.solve_dense(torch.zeros((224, 1), dtype=torch.int32, device="cuda"))


def test_windows_side_by_side_in_one_array_are_no_overlap(S):
    """B = W[:, :K] and X = W[:N, K:2K] interleave in memory without sharing a word: both entries take them, on the device and on
    the host, and leave the rest of W alone.  Windows that share one word are refused by Python (ValueError) and, asked directly, by
    the engine (-1, nothing written)."""
    import torch

    rng = np.random.default_rng(1913)
    p = 65521
    K = 7
    systems = [system(rng, 20, 24, K, p) + (p,), system(rng, 9, 30, K, p) + (p,)]
    Xw, okw, _, _ = run_list(S, systems, rng)
    raw = [balanced(B, q) for _, B, q in systems]
    mats = [csr_of(S, balanced(A, q), A != 0, q, rng) for A, _, q in systems]
    Bd = np.concatenate([R.T for R in raw], axis=0).astype(np.int32)
    M, N = 54, 29
    Wh = np.full((M, 2 * K + 2), SENTINEL, dtype=np.int32)
    Wh[:, :K] = Bd
    with S.BatchSolver(mats) as sv:
        W = to_dev(Wh)
        X, ok = sv.solve_dense(W[:, :K], X=W[:N, K:2 * K])
        got = W.cpu().numpy()
        assert np.array_equal(got[:N, K:2 * K], Xw) and np.array_equal(ok.cpu().numpy(), okw)
        assert np.array_equal(got[:, :K], Bd) and (got[N:, K:] == SENTINEL).all() and (got[:, 2 * K:] == SENTINEL).all()
        Wn = Wh.copy()
        Xn, okn = sv.solve_dense(Wn[:, :K], X=Wn[:N, K:2 * K])
        assert np.array_equal(Wn, got) and np.array_equal(okn, okw)
        # one shared word: the last word of row 0 of B is the first of row 0 of X
        keep = W.clone()
        with pytest.raises(ValueError, match="overlap"):
            sv.solve_dense(W[:, :K], X=W[:N, K - 1:2 * K - 1])
        with pytest.raises(ValueError, match="overlap"):
            sv.solve_dense(Wn[:, :K], X=Wn[:N, K - 1:2 * K - 1])
        okt = torch.full((2 * K,), 0xA5, dtype=torch.uint8, device="cuda")
        rc = S._abi.lib().spasm_amd_solver_apply_dense_dev(sv._need(), K, C.c_void_p(W.data_ptr()), 2 * K + 2, C.c_void_p(W.data_ptr() + 4 * (K - 1)), 2 * K + 2,
                                                           C.c_void_p(okt.data_ptr()), None)
        assert rc == -1 and "spasm_amd_solver_apply_dense_dev: B and X overlap" in S._abi.last_error()
        assert torch.equal(W, keep) and bool((okt == 0xA5).all())


def test_a_plan_is_not_rebuilt_on_a_capturing_stream(S):
    """An apply whose K is not the K of the cached plan would have to wait for the device and copy on the NULL stream; while its
    stream is capturing it is refused before anything is touched, the capture stays valid, and the handle goes on working."""
    import torch

    rng = np.random.default_rng(1912)
    p = 65521
    K = 6
    A, B = system(rng, 20, 24, K, p)
    Ac = csr_of(S, balanced(A, p), A != 0, p, rng)
    Bt = to_dev(balanced(B, p).T.astype(np.int32))
    B4 = Bt[:, :4].contiguous()
    X4 = torch.full((20, 4), SENTINEL, dtype=torch.int32, device="cuda")
    with S.BatchSolver([Ac]) as sv:
        X, ok = sv.solve_dense(Bt)
        Xh, okh = X.cpu().numpy(), ok.cpu().numpy()
        assert okh.any() and not okh.all()
        count = torch.zeros(4, dtype=torch.int32, device="cuda")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            count.add_(1)
            with pytest.raises(S.SpasmError, match="spasm_amd_solver_apply_dense_dev: the stream is capturing .* K = 4"):
                sv.solve_dense(B4, X=X4)
            count.add_(1)
        torch.cuda.synchronize()
        assert bool((X4 == SENTINEL).all())
        assert (sv.dense_info()["plan_k"], sv.dense_info()["plans_built"]) == (K, 1)
        X2, ok2 = sv.solve_dense(B4, X=X4)                     # outside the capture the same call rebuilds the plan
        assert np.array_equal(X2.cpu().numpy(), Xh[:, :4]) and np.array_equal(ok2.cpu().numpy(), okh[:, :4])
        assert sv.dense_info()["plans_built"] == 2


def test_the_split_of_a_matrix_without_rows_and_columns(S):
    """no system, no row of B or X, and still K flags: 0 = 0 holds for every column, on the device and through the host entry"""
    import torch

    A = S.CSR.from_arrays(0, 0, np.array([0], dtype=np.int64), np.array([], dtype=np.int32), np.array([], dtype=np.int32), prime=127)
    with S.DeviceBlocks(A) as db:
        sv = db.solver()
    with sv:
        assert len(sv) == 0 and (sv.dense_info()["rows"], sv.dense_info()["cols"], sv.dense_info()["ok_rows"]) == (0, 0, 1)
        X, ok = sv.solve_dense(torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
        assert tuple(X.shape) == (0, 3) and ok.cpu().numpy().tolist() == [True, True, True]
        Xn, okn = sv.solve_dense(np.zeros((0, 3), dtype=np.int32))
        assert Xn.shape == (0, 3) and okn.tolist() == [True, True, True]
        assert sv.dense_info()["plans_built"] == 1            # (the host entry needs neither a plan nor a device)
