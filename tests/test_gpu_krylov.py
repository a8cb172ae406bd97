"""GPU tests of the projected Krylov sequence and of Berlekamp-Massey (spasm_amd_krylov_sequence / _dev, spasm_amd_berlekamp_massey;
csrc/krylov.hpp).  Every comparison is exact, against the references of tests/wiedemann_ref.py (numpy int64 with the split mulmod)."""
import ctypes as C

import numpy as np
import pytest

import wiedemann_ref as W
from wiedemann_ref import PRIMES, bal

pytestmark = pytest.mark.gpu

P16, P31, P32 = 65521, 2**31 - 1, 4294967291
SENTINEL = 0x5A5A5A5A


def rand_bal(rng, shape, p):
    return bal(rng.integers(0, p, size=shape, dtype=np.int64), p)


def mixed_matrix(rng, n, p):
    """n x n with rows of length 0, 1, 32 (the last short one), 33 (the first medium one) and a few others, in random places"""
    lens = rng.choice([0, 1, 5, 32, 33, 70], size=n, p=[0.15, 0.25, 0.2, 0.15, 0.15, 0.1])
    lens[:6] = [0, 1, 32, 33, 70, 0]
    rows = []
    for l in lens:
        cols = rng.choice(n, size=int(l), replace=False)
        rows.append([(int(c), int(v)) for c, v in zip(cols, rng.integers(1, p, size=int(l)))])
    return W.Mat.from_rows(rows, n)


def long_rows_matrix(rng, n, p):
    """row 3 has 16385 entries (two segments, the second of one entry), row 7 all n = 40000 (three segments), the others 0 .. 3"""
    rows = []
    for i in range(n):
        l = 16385 if i == 3 else n if i == 7 else int(rng.integers(0, 4))
        cols = rng.choice(n, size=l, replace=False) if l < n else np.arange(n)
        rows.append(list(zip(cols.tolist(), rng.integers(1, p, size=l).tolist())))
    return W.Mat.from_rows(rows, n)


def run_seq(S, M, p, U, V, length, trans=False, reduce=True):
    with S.SpMV(M.csr(S, p, reduce=reduce)) as op:
        return S.krylov_sequence(op, U, V, length, trans=trans)


@pytest.mark.parametrize("p", PRIMES)
def test_one_by_one_and_zero_matrix(S, p):
    rng = np.random.default_rng(11 + p % 1000)
    a = int(rng.integers(1, p))
    M = W.Mat.from_rows([[(0, a)]], 1)
    U, V = rand_bal(rng, (1, 3), p), rand_bal(rng, (1, 3), p)
    assert run_seq(S, M, p, U, V, 8).tolist() == W.ref_sequence(M, U, V, 8, p).tolist()
    # one vector given as a 1-d array
    got = run_seq(S, M, p, U[:, 0].copy(), V[:, 0].copy(), 5)
    assert got.shape == (5, 1) and got[:, 0].tolist() == W.ref_sequence(M, U[:, :1], V[:, :1], 5, p)[:, 0].tolist()
    # every row is short, so the short class runs over the row range without a list: every chunk width KW of that launch, on the
    # permutation-like matrix of the worst-case test below at n = 300 with random entries (several teams a workgroup, several
    # workgroups; a wrong row or team stride moves an entry)
    n = 300
    P = W.Mat(n, n, np.arange(n + 1), rng.permutation(n), rng.integers(1, p, size=n))
    for K in (1, 2, 4, 8, 16, 32, 64):
        U, V = rand_bal(rng, (n, K), p), rand_bal(rng, (n, K), p)
        assert run_seq(S, P, p, U, V, 4).tolist() == W.ref_sequence(P, U, V, 4, p).tolist(), K
    # the zero matrix: s_0 = u . v, then zeros
    n = 300
    Z = W.Mat.from_rows([[] for _ in range(n)], n)
    U, V = rand_bal(rng, (n, 8), p), rand_bal(rng, (n, 8), p)
    got = run_seq(S, Z, p, U, V, 6)
    want = W.ref_sequence(Z, U, V, 6, p)
    assert got.tolist() == want.tolist() and not got[1:].any()
    assert p == 3 or got[0].any()


@pytest.mark.parametrize("trans", (False, True))
@pytest.mark.parametrize("K", (1, 2, 3, 8, 16, 32, 64))   # every chunk width KW = 1, 2, 4, .., 64 of the step kernel
@pytest.mark.parametrize("p", PRIMES)
def test_short_and_medium_rows_many_workgroups(S, p, K, trans):
    rng = np.random.default_rng(1000 * K + p % 997 + int(trans))
    n = 1000
    M = mixed_matrix(rng, n, p)
    U, V = rand_bal(rng, (n, K), p), rand_bal(rng, (n, K), p)
    V0 = V.copy()
    want = W.ref_sequence(M, U, V, 8, p, trans=trans)
    with S.SpMV(M.csr(S, p)) as op:
        got = S.krylov_sequence(op, U, V, 8, trans=trans)
        again = S.krylov_sequence(op, U, V, 8, trans=trans)
    assert got.shape == (8, K) and got.dtype == np.int32
    assert got.tolist() == want.tolist()
    assert again.tobytes() == got.tobytes()
    assert V.tobytes() == V0.tobytes()


@pytest.mark.parametrize("trans", (False, True))
@pytest.mark.parametrize("p,K", [(3, 8), (127, 1), (P16, 8), (P31, 3), (P32, 8), (P32, 64),
                                 # the other widths of either accumulator: i32 (p < 2^16) with KW = 2, 4, 16, 32, 64, i64 with 1, 2, 16, 32
                                 (P16, 2), (3, 4), (127, 16), (P16, 32), (3, 64), (P32, 1), (P31, 2), (P32, 16), (P31, 32)])
def test_long_rows_carry_the_projection_in_the_combine(S, p, K, trans):
    rng = np.random.default_rng(77 + K + p % 991)
    n = 40000
    M = long_rows_matrix(rng, n, p)
    U, V = rand_bal(rng, (n, K), p), rand_bal(rng, (n, K), p)
    want = W.ref_sequence(M, U, V, 4, p, trans=trans)
    got = run_seq(S, M, p, U, V, 4, trans=trans)
    assert got.tolist() == want.tolist()


@pytest.mark.parametrize("p", PRIMES)
def test_worst_case_of_the_64_bit_projection_sum(S, p):
    """every entry of U, of V and of the permutation-like A is halfp (or mhalfp): A^i V is a constant vector, so the n = 70000
    terms of a projection are one and the same residue and nothing cancels in the integer sum (n * |term|, up to 2^47)"""
    n, K, hp = 70000, 8, p // 2
    perm = np.random.default_rng(5).permutation(n)
    for sign in (1, -1):
        M = W.Mat(n, n, np.arange(n + 1), perm, np.full(n, sign * hp))
        U = np.full((n, K), hp, dtype=np.int32)
        V = np.full((n, K), sign * hp, dtype=np.int32)
        want = W.ref_sequence(M, U, V, 4, p)
        got = run_seq(S, M, p, U, V, 4)
        assert got.tolist() == want.tolist(), sign


@pytest.mark.parametrize("p", (3, P16, P31))
def test_unreduced_inputs_and_the_sentinel_behind_S(S, p):
    rng = np.random.default_rng(31 + p % 100)
    n, K, length = 500, 3, 6
    M = mixed_matrix(rng, n, p)
    lift = lambda a: (a.astype(np.int64) + p * rng.integers(-(2**31 - 1 - p) // p, (2**31 - 1 - p) // p + 1, size=a.shape)).astype(np.int32)
    Mr = W.Mat(M.n, M.m, M.ptr, M.j, lift(bal(M.v, p)))
    U, V = lift(rand_bal(rng, (n, K), p)), lift(rand_bal(rng, (n, K), p))
    want = W.ref_sequence(M, U, V, length, p)
    # through the C entry, with U and V at a leading dimension above K and a sentinel behind S
    ld = K + 2
    Ub, Vb = np.full((n, ld), SENTINEL, dtype=np.int32), np.full((n, ld), SENTINEL, dtype=np.int32)
    Ub[:, :K], Vb[:, :K] = U, V
    Sbuf = np.full(length * K + 16, SENTINEL, dtype=np.int32)
    with S.SpMV(Mr.csr(S, p, reduce=False)) as op:
        rc = S._abi.lib().spasm_amd_krylov_sequence(op._op, 0, K, length, Ub.ctypes.data, ld, Vb.ctypes.data, ld, Sbuf.ctypes.data)
        assert rc == 0, S._abi.last_error()
        # len == 0 succeeds and writes nothing
        assert S._abi.lib().spasm_amd_krylov_sequence(op._op, 0, K, 0, Ub.ctypes.data, ld, Vb.ctypes.data, ld, Sbuf.ctypes.data + 4 * length * K) == 0
        with pytest.raises(S.SpasmError, match="K out of range"):
            S.krylov_sequence(op, np.zeros((n, 65), dtype=np.int32), np.zeros((n, 65), dtype=np.int32), 2)
    assert Sbuf[: length * K].reshape(length, K).tolist() == want.tolist()
    assert (Sbuf[length * K:] == SENTINEL).all()
    assert (Vb[:, :K] == V).all() and (Vb[:, K:] == SENTINEL).all()
    st = S.minpoly_stats()
    assert st["n"] == 0 and st["steps"] == 0   # the failed call cleared the counters


def test_stats_and_a_matrix_that_is_not_square(S):
    p, n, K = P16, 1000, 8
    rng = np.random.default_rng(3)
    M = mixed_matrix(rng, n, p)
    with S.SpMV(M.csr(S, p)) as op:
        S.krylov_sequence(op, rand_bal(rng, (n, K), p), rand_bal(rng, (n, K), p), 5)
        st = S.minpoly_stats()
    # s_0, then per step one launch for the short rows and one for the medium rows, then the residues
    assert (st["n"], st["K"], st["steps"], st["launches"]) == (n, K, 4, 1 + 4 * 2 + 1)
    T = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=127)
    with S.SpMV(T) as op:
        with pytest.raises(S.SpasmError, match=r"not square \(3 x 2\)"):
            S.krylov_sequence(op, np.zeros((3, 1), dtype=np.int32), np.zeros((3, 1), dtype=np.int32), 2)


@pytest.mark.parametrize("trans", (False, True))
@pytest.mark.parametrize("p,K", [(3, 3), (P16, 8), (P32, 1), (P32, 64)])
def test_dev_entry_on_torch_tensors_gives_the_same_bytes(S, p, K, trans):
    import torch

    rng = np.random.default_rng(19 + K)
    n = 1000
    M = mixed_matrix(rng, n, p)
    U, V = rand_bal(rng, (n, K), p), rand_bal(rng, (n, K), p)
    with S.SpMV(M.csr(S, p)) as op:
        host = S.krylov_sequence(op, U, V, 7, trans=trans)
        Ut, Vt = torch.from_numpy(U).cuda(), torch.from_numpy(V).cuda()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            St = S.krylov_sequence(op, Ut, Vt, 7, trans=trans)
        side.synchronize()
        dev = St.cpu().numpy()
        assert torch.equal(Vt.cpu(), torch.from_numpy(V))
    assert dev.tobytes() == host.tobytes()
    assert host.tolist() == W.ref_sequence(M, U, V, 7, p, trans=trans).tolist()


# ---------------------------------------------------------------------------------------------
# Berlekamp-Massey
# ---------------------------------------------------------------------------------------------
def check_recurrence(s, f, p):
    """f (low degree first, degree L) annihilates s: sum_k f[k] s[i + k] = 0 for all i with i + L < len(s)"""
    L = len(f) - 1
    for i in range(len(s) - L):
        assert sum(int(f[k]) * int(s[i + k]) for k in range(L + 1)) % p == 0, i


@pytest.mark.parametrize("p", PRIMES)
def test_bm_small_sequences(S, p):
    assert S.berlekamp_massey([0, 0, 0, 0, 0, 0], p).tolist() == [1]
    assert S.berlekamp_massey([1, 0, 0, 0], p).tolist() == [0, 1]
    # 0, 0, 0, 1: 2 L > len, the polynomial is not unique; L and the recurrence are
    f = S.berlekamp_massey([0, 0, 0, 1], p)
    assert len(f) - 1 == 4 == W.ref_bm([0, 0, 0, 1], p)[1] and f[-1] == 1
    check_recurrence([0, 0, 0, 1], f, p)
    fib = [0, 1]
    while len(fib) < 12:
        fib.append((fib[-1] + fib[-2]) % p)
    assert S.berlekamp_massey(fib, p).tolist() == bal([-1, -1, 1], p).tolist()
    # leading zeros: the length jumps with m > 1
    for z in (1, 2, 5):
        s = [0] * z + [int(x) for x in W.lfsr_sequence([3 % p or 1, 1, 1], [1, 2], 14, p)]
        want, L = W.ref_bm(s, p)
        got = S.berlekamp_massey(s, p)
        assert got.tolist() == bal(want, p).tolist(), z
        check_recurrence(s, got, p)
    assert S.berlekamp_massey(np.zeros((4, 0), dtype=np.int32), p) == []
    assert S.berlekamp_massey(np.zeros(0, dtype=np.int32), p).tolist() == [1]   # len == 0


@pytest.mark.parametrize("d", (1, 2, 255, 256, 257, 600))
@pytest.mark.parametrize("p", PRIMES)
def test_bm_companion_sequences_byte_for_byte_in_both_classes(S, p, d):
    rng = np.random.default_rng(100 * d + p % 977)
    # nine sequences of 2 d terms: the recurrences of random monic polynomials of degree d from random starts, one of them zero
    # and one shifted by leading zeros
    cols, want = [], []
    for c in range(9):
        f = W.rand_monic(rng, d, p)
        s = W.lfsr_sequence(f, rng.integers(0, p, size=d), 2 * d, p)
        if c == 4:
            s[:] = 0
        if c == 6:
            s[: d // 2 + 1] = 0
        cols.append(s)
        g, L = W.ref_bm(s, p)
        want.append(bal(g, p))
        if c not in (4, 6) and L == d:
            assert g == [int(x) % p for x in f]   # 2 d terms fix the recurrence of degree d
    Sq = bal(np.stack(cols, axis=1), p)
    for count in (9, 1):
        res = {}
        for where in (0, 1, 2):
            got = S.berlekamp_massey(Sq[:, :count], p, where=where)
            assert len(got) == count
            for c in range(count):
                assert got[c].tolist() == want[c].tolist(), (where, c)
            res[where] = b"".join(g.tobytes() for g in got)
            assert S.minpoly_stats()["bm_class"] == (2 if where == 2 else 1)
        assert res[0] == res[1] == res[2]


def test_bm_longest_sequence_of_the_lds_class(S):
    """len = 20223: 2 * (len + 1) words are all the LDS the class takes; one term more goes to device memory"""
    p, d, length = P32, 40, 20223
    rng = np.random.default_rng(8)
    f = W.rand_monic(rng, d, p)
    s = np.concatenate([np.zeros(7, dtype=np.int64), W.lfsr_sequence(f, rng.integers(0, p, size=d), length - 7, p)])
    want, L = W.ref_bm(s, p)
    assert L == d + 7
    a = S.berlekamp_massey(s, p, where=1)
    assert S.minpoly_stats()["bm_class"] == 1
    b = S.berlekamp_massey(s, p, where=2)
    assert a.tolist() == bal(want, p).tolist() and a.tobytes() == b.tobytes()
    S.berlekamp_massey(np.append(s, 0), p)
    assert S.minpoly_stats()["bm_class"] == 2
    with pytest.raises(S.SpasmError, match=r"the LDS class does not fit \(len = 20224, at most 20223\)"):
        S.berlekamp_massey(np.append(s, 0), p, where=1)


def test_bm_rows_are_zeroed_above_the_degree_and_unreduced_terms(S):
    p, length, count = 127, 10, 3
    rng = np.random.default_rng(9)
    s = np.stack([W.lfsr_sequence([5, 7, 1], [1, 1], length, p), np.zeros(length, dtype=np.int64), W.lfsr_sequence([2, 1], [9], length, p)], axis=1)
    raw = (s + p * rng.integers(-1000, 1000, size=s.shape)).astype(np.int32)
    lds, ldc = count + 2, length + 3
    Sb = np.full((length, lds), SENTINEL, dtype=np.int32)
    Sb[:, :count] = raw
    coef = np.full(count * ldc + 8, SENTINEL, dtype=np.int32)
    deg = np.full(count + 2, SENTINEL, dtype=np.int32)
    rc = S._abi.lib().spasm_amd_berlekamp_massey(count, length, Sb.ctypes.data, lds, p, 0, coef.ctypes.data, ldc, deg.ctypes.data)
    assert rc == 0, S._abi.last_error()
    assert deg[:count].tolist() == [2, 0, 1] and (deg[count:] == SENTINEL).all()
    rows = coef[: count * ldc].reshape(count, ldc)
    assert rows[0].tolist() == [5, 7, 1] + [0] * (ldc - 3)
    assert rows[1].tolist() == [1] + [0] * (ldc - 1)
    assert rows[2].tolist() == [2, 1] + [0] * (ldc - 2)
    assert (coef[count * ldc:] == SENTINEL).all()
