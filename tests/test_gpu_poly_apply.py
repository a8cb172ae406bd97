"""GPU tests of spasm_amd_poly_apply / _poly_apply_dev (csrc/horner.hpp): a polynomial of the resident exact product applied to
vectors, one fused Horner step Y <- A X + c B per product.  Every comparison is byte for byte against Horner through Mat.apply on
the host (tests/wiedemann_solve_ref.py).  One matrix holds every row class of the operator."""
import functools

import numpy as np
import pytest

import sparse_worst_cases as SW
import wiedemann_ref as W
from wiedemann_ref import bal
from wiedemann_solve_ref import ref_poly_apply

pytestmark = pytest.mark.gpu

P16, P31, P32 = 65521, 2**31 - 1, 4294967291
PRIMES = (3, P16, 65537, P31, P32)
KS = (1, 2, 3, 8, 16, 32, 33, 64)   # every chunk width KW = 1, 2, 4, .., 64 of the step kernel; 3 and 33 leave columns idle
SENTINEL = 0x5A5A5A5A
N = 32770
SPECIAL = {0: 0, 1: 1, 2: 32, 3: 33, 4: 16384, 5: 16385, 6: 2 * 16384 + 1, 7: 0}   # row -> length; the other rows are short
DEGREES = (5, -1, 0, 1)


@functools.lru_cache(maxsize=None)
def structure():
    """(ptr, columns) of the n = 32770 matrix: empty rows, rows of 1, 32 (the last short), 33 (the first medium), 16384 (the last
    medium), 16385 (two segments, the second of one entry) and 2 * 16384 + 1 entries (three segments), the remaining rows 0 .. 3;
    the columns of a row are distinct and stored unsorted"""
    rng = np.random.default_rng(20)
    lengths = rng.integers(0, 4, size=N)
    for r, l in SPECIAL.items():
        lengths[r] = l
    ptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(lengths, out=ptr[1:])
    row = np.repeat(np.arange(N), lengths)
    cols = (row * 7 + (np.arange(ptr[-1]) - ptr[row]) * 1009 + 13) % N
    for r, l in SPECIAL.items():
        cols[ptr[r]: ptr[r + 1]] = rng.choice(N, size=l, replace=False)
    return ptr, cols


def all_classes(p):
    ptr, cols = structure()
    return W.Mat(N, N, ptr, cols, SW.rand_values(p, len(cols), np.random.default_rng(21 + p % 1009)))


def launches_per_product(M):
    l = np.diff(M.ptr)
    return int((l <= 32).any()) + int(((l > 32) & (l <= 16384)).any()) + 2 * int((l > 16384).any())


def polys_for(rng, K, p):
    """degrees 5, -1, 0, 1 in turn, mixed within one call; any coefficient, the leading one not zero"""
    out = []
    for c in range(K):
        d = DEGREES[c % 4]
        f = rng.integers(0, p, size=d + 1, dtype=np.int64)
        if d >= 0:
            f[-1] = f[-1] or 1
        out.append(bal(f, p))
    return out


@pytest.fixture(scope="module")
def ops(S):
    """p -> (the matrix, its transpose, the resident operator), built once and shared"""
    made = {}

    def get(p):
        if p not in made:
            M = all_classes(p)
            made[p] = (M, M.transpose(), S.SpMV(M.csr(S, p)))
        return made[p]

    yield get
    for _, _, op in made.values():
        op.close()


@pytest.mark.parametrize("trans", (False, True))
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("p", PRIMES)
def test_every_row_class_mixed_degrees(S, ops, p, K, trans):
    M, Mt, op = ops(p)
    rng = np.random.default_rng(100 * K + p % 997 + int(trans))
    V = bal(rng.integers(0, p, size=(N, K), dtype=np.int64), p)
    V0 = V.copy()
    polys = polys_for(rng, K, p)
    want = ref_poly_apply(Mt if trans else M, polys, V, p)
    got = S.poly_apply(op, polys, V, trans=trans)
    st = S.wiedemann_stats()
    assert got.dtype == np.int32 and got.shape == (N, K)
    assert got.tobytes() == want.tobytes()
    assert S.poly_apply(op, polys, V, trans=trans).tobytes() == got.tobytes()   # two runs, the same bytes
    assert V.tobytes() == V0.tobytes()
    # max(deg) = 5 products, one launch per non-empty row class each (A has all: short, medium, long segments + combine; the rows
    # of its transpose are all short); one scale first
    assert launches_per_product(M) == 4 and launches_per_product(Mt) == 1
    assert (st["n"], st["K"], st["products"], st["launches"]) == (N, K, 5, 1 + 5 * launches_per_product(Mt if trans else M))
    for c in range(K):
        if DEGREES[c % 4] == -1:
            assert not got[:, c].any()


@pytest.mark.parametrize("p", PRIMES)
def test_zero_and_constant_polynomials_alone(S, ops, p):
    M, _, op = ops(p)
    rng = np.random.default_rng(5 + p % 991)
    V = bal(rng.integers(0, p, size=(N, 3), dtype=np.int64), p)
    assert not S.poly_apply(op, [[], [], []], V).any()
    assert S.wiedemann_stats()["products"] == 0 and S.wiedemann_stats()["launches"] == 0
    consts = [[2], [], [-1]]
    got = S.poly_apply(op, consts, V)
    assert got.tobytes() == ref_poly_apply(M, consts, V, p).tobytes()
    assert S.wiedemann_stats()["products"] == 0 and S.wiedemann_stats()["launches"] == 1
    # one vector, one polynomial
    f = [1, 2, 3]
    got = S.poly_apply(op, f, V[:, 0].copy())
    assert got.shape == (N,) and got.tobytes() == ref_poly_apply(M, [f], V[:, :1], p)[:, 0].tobytes()


@pytest.mark.parametrize("pattern", ("equal", "alternating"))
@pytest.mark.parametrize("p", PRIMES)
def test_worst_case_accumulators(S, p, pattern):
    """every entry of A, every coefficient and every entry of V is +-floor(p / 2): the lazy sums of the long rows (16384 terms a
    segment) and c * b are as large as they get; all of one sign, and alternating"""
    hp = p // 2
    ptr, cols = structure()
    alt = pattern == "alternating"
    sign = lambda count: np.where(np.arange(count) % 2 == 1, -1, 1) if alt else np.ones(count, dtype=np.int64)
    M = W.Mat(N, N, ptr, cols, hp * sign(len(cols)))
    K = 8
    V = (hp * sign(N))[:, None].repeat(K, axis=1).astype(np.int32)
    polys = [(hp * sign(DEGREES[c % 4] + 1)).astype(np.int32) for c in range(K)]
    with S.SpMV(M.csr(S, p)) as op:
        for trans in (False, True):
            want = ref_poly_apply(M.transpose() if trans else M, polys, V, p)
            assert S.poly_apply(op, polys, V, trans=trans).tobytes() == want.tobytes(), trans


@pytest.mark.parametrize("p", PRIMES)
def test_unreduced_int32_inputs_and_leading_dimensions(S, ops, p):
    M, _, op = ops(p)
    rng = np.random.default_rng(31 + p % 100)
    K, ldv, ldx, ldc = 3, 5, 4, 8
    V = SW.rand_int32(rng, (N, K))
    V[0, 0], V[1, 0] = -2**31, 2**31 - 1
    polys = [np.array([-2**31, 2**31 - 1, 7, -2**31, 2**31 - 1, 2**31 - 1], dtype=np.int32), np.array([2**31 - 1], dtype=np.int32),
             np.array([-2**31, -2**31], dtype=np.int32)]
    want = ref_poly_apply(M, polys, V, p)
    assert S.poly_apply(op, polys, V).tobytes() == want.tobytes()
    # through the C entry: leading dimensions above K, sentinels in the gaps
    Vb = np.full((N, ldv), SENTINEL, dtype=np.int32)
    Vb[:, :K] = V
    Xb = np.full((N, ldx), SENTINEL, dtype=np.int32)
    coef = np.full((K, ldc), SENTINEL, dtype=np.int32)
    for c, f in enumerate(polys):
        coef[c, : len(f)] = f
    deg = np.array([len(f) - 1 for f in polys], dtype=np.int32)
    lib = S._abi.lib()
    rc = lib.spasm_amd_poly_apply(op._op, 0, K, deg.ctypes.data, coef.ctypes.data, ldc, Vb.ctypes.data, ldv, Xb.ctypes.data, ldx)
    assert rc == 0, S._abi.last_error()
    assert Xb[:, :K].tobytes() == want.tobytes() and (Xb[:, K:] == SENTINEL).all()
    assert (Vb[:, :K] == V).all() and (Vb[:, K:] == SENTINEL).all()


def test_argument_errors_write_nothing(S, ops):
    _, _, op = ops(P16)
    lib, err = S._abi.lib(), S._abi.last_error
    K = 2
    V = np.ones((N, K), dtype=np.int32)
    X = np.full((N, K), SENTINEL, dtype=np.int32)
    coef = np.ones((K, 4), dtype=np.int32)
    deg = np.array([3, 1], dtype=np.int32)
    call = lambda K=K, deg=deg, coef=coef, ldc=4, V=V, ldv=K, X=X, ldx=K, trans=0: lib.spasm_amd_poly_apply(
        op._op, trans, K, None if deg is None else deg.ctypes.data, None if coef is None else coef.ctypes.data, ldc,
        None if V is None else V.ctypes.data, ldv, None if X is None else X.ctypes.data, ldx)
    for k in (0, 65):
        assert call(K=k, ldv=65, ldx=65) == -1 and err() == "spasm_amd_poly_apply: K out of range (1 <= K <= 64)"
    assert call(trans=2) == -1 and err() == "spasm_amd_poly_apply: trans must be 0 or 1"
    assert call(ldv=1) == -1 and err() == "spasm_amd_poly_apply: ldv < K"
    assert call(ldx=1) == -1 and err() == "spasm_amd_poly_apply: ldx < K"
    assert call(ldc=3) == -1 and err() == "spasm_amd_poly_apply: polynomial 0: ldc < deg + 1 (ldc = 3, deg = 3)"
    assert call(deg=np.array([3, -2], dtype=np.int32)) == -1 and err() == "spasm_amd_poly_apply: polynomial 1: a degree below -1 (-2)"
    for miss in ("deg", "coef", "V", "X"):
        assert call(**{miss: None}) == -1 and err() == "spasm_amd_poly_apply: NULL array", miss
    both = np.ones((N + 1, K), dtype=np.int32)
    assert call(V=both[:N], X=both[1:]) == -1 and err() == "spasm_amd_poly_apply: V must not overlap X"
    assert (X == SENTINEL).all()
    assert not any(S.wiedemann_stats().values())
    tall = S.CSR.from_rows([[(0, 1), (1, 2)], [(1, -3)], []], 2, prime=127)
    with S.SpMV(tall) as top:
        with pytest.raises(S.SpasmError, match=r"spasm_amd_poly_apply: not square \(3 x 2\)"):
            S.poly_apply(top, [[1]], np.zeros((3, 1), dtype=np.int32))


@pytest.mark.parametrize("p", (P16, P32))
def test_torch_entry_on_a_side_stream_gives_the_numpy_bytes(S, ops, p):
    import torch

    M, Mt, op = ops(p)
    rng = np.random.default_rng(77 + p % 13)
    K = 8
    V = bal(rng.integers(0, p, size=(N, K), dtype=np.int64), p)
    polys = polys_for(rng, K, p)
    for trans in (False, True):
        want = S.poly_apply(op, polys, V, trans=trans)
        A = Mt if trans else M
        wantY = bal(A.apply(want.astype(np.int64) % p, p), p)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            Vt = torch.from_numpy(V).cuda()
            Yt = torch.zeros((N, K), dtype=torch.int32, device="cuda")
            Xt = S.poly_apply(op, polys, Vt, trans=trans)
            op.apply(Xt, Yt, trans=trans)   # no synchronize in between: the product queues behind the Horner run
        side.synchronize()
        assert Xt.cpu().numpy().tobytes() == want.tobytes(), trans
        assert Yt.cpu().numpy().tobytes() == wantY.tobytes(), trans


@pytest.mark.parametrize("p", (3, P16, P31, P32))
def test_the_minimal_polynomial_of_the_hidden_companions_annihilates(S, p):
    """C(f1) + C(f2) + C(f1) under a simultaneous permutation of rows and columns: its minimal polynomial f1 f2 applied to any
    vectors gives 0, and one factor alone does not"""
    rng = np.random.default_rng(4242 + p % 1009)
    while True:
        f1, f2 = W.rand_monic(rng, 7, p), W.rand_monic(rng, 12, p)
        if f1[0] and f2[0] and W.pgcd(f1, f2, p) == [1]:
            break
    D = W.block_diag([W.companion(f1, p), W.companion(f2, p), W.companion(f1, p)])
    perm = rng.permutation(len(D))
    M = W.Mat.from_dense(D[np.ix_(perm, perm)])
    mp = bal(W.pmul(f1, f2, p), p)
    V = bal(rng.integers(0, p, size=(M.n, 4), dtype=np.int64), p)
    V[:, 3] = 0
    V[0, 3] = 1
    with S.SpMV(M.csr(S, p)) as op:
        for trans in (False, True):
            assert not S.poly_apply(op, [mp] * 4, V, trans=trans).any(), trans
        part = S.poly_apply(op, [bal(f1, p)] * 4, V)
        assert part.tobytes() == ref_poly_apply(M, [f1] * 4, V, p).tobytes() and part.any()
