"""The 32-bit lazy accumulators of the sparse path at their worst case: equal-sign terms of the largest magnitude.

For p < 2^16 the kernels sum lazy products |t| <= halfp + 256 (csrc/zp.hpp) in i32 and reduce once at the end, so an accumulator
holds cap(p) = floor((2^31 - 1) / (halfp + 256)) terms: 65043 for p = 65521.  Random values never get near that (their partial
sums grow like sqrt(N) * p); the matrices here make every term on one column +halfp, or every term -halfp.  A sum that wraps
mod 2^32 is not a multiple of p off, so the Schur entry comes out wrong and no counter says so.  Everything is compared with
closed forms in Python integers; the CPU oracle is a second reference where it takes part."""
import ctypes as C

import numpy as np
import pytest
from conftest import LM
from test_gpu_parity import run_plan

pytestmark = pytest.mark.gpu


def balanced(x, p):
    r = x % p
    return r - p if r > p // 2 else r


def lazy_capacity(p):
    """Lazy terms an i32 accumulator holds without wrapping (csrc/zp.hpp, zp_lazy_terms without its 2^20 ceiling)."""
    return (2**31 - 1) // (p // 2 + 256)


# ---- (a), (b): a bidiagonal chain whose multipliers are all +1 (or all -1) ------------------------------------------------------

def chain_matrix(S, p, N, m):
    """Pivot rows i = 0..N-1: {i: 1, i+1: -1, C: h} with h = halfp, C = N + 1 (column N stays free); two probe rows
    {0: s, N+2: 1, N+3: 1, N+4: 1}, s = +1 and s = -1, longer than the pivot rows so that they are never elected.
    Eliminating column i of a probe row takes the multiplier s and puts s on column i + 1: every multiplier is s, every term
    on column C is -s * h."""
    assert m >= N + 5
    h = p // 2
    n = N + 2
    ptr = np.empty(n + 1, dtype=np.int64)
    ptr[: N + 1] = 3 * np.arange(N + 1)
    ptr[N + 1] = 3 * N + 4
    ptr[N + 2] = 3 * N + 8
    j = np.empty(3 * N + 8, dtype=np.int32)
    x = np.empty(3 * N + 8, dtype=np.int32)
    i = np.arange(N)
    j[0:3 * N:3], j[1:3 * N:3], j[2:3 * N:3] = i, i + 1, N + 1
    x[0:3 * N:3], x[1:3 * N:3], x[2:3 * N:3] = 1, -1, h
    for k, s in enumerate((1, -1)):
        j[3 * N + 4 * k: 3 * N + 4 * k + 4] = [0, N + 2, N + 3, N + 4]
        x[3 * N + 4 * k: 3 * N + 4 * k + 4] = [s, 1, 1, 1]
    return S.CSR.from_arrays(n, m, ptr, j, x, prime=p)


def chain_expected(p, N):
    """The two Schur rows, exact: s on column N, -s * N * h on column C = N + 1, the three ones untouched."""
    h = p // 2
    rows = []
    for s in (1, -1):
        row = [(N, s), (N + 1, balanced(-s * N * h, p)), (N + 2, 1), (N + 3, 1), (N + 4, 1)]
        rows.append([(c, v) for c, v in row if v != 0])
    return rows


CHAIN_CASES = [
    # id, p, N, m - N, i32 tables, last-resort class: None = either (how a row beyond the capacity is kept exact is the engine's choice)
    ("p65521_60000_below_capacity", 65521, 60000, 5, True, False),
    ("p65521_70000_above_capacity", 65521, 70000, 5, True, None),
    ("p65521_70000_global_memory_class", 65521, 70000, 70011, True, True),
    ("p32749_70000_capacity_129k", 32749, 70000, 5, True, False),
    ("p65537_70000_i64_tables", 65537, 70000, 5, False, False),
]


@pytest.mark.parametrize("name,p,N,extra,small,big", CHAIN_CASES, ids=[c[0] for c in CHAIN_CASES])
def test_schur_round_equal_sign_chain(S, O, name, p, N, extra, small, big):
    """One Schur round of chain_matrix.  With m = N + 5 only 5 columns are free, the bound of the Schur row is capped at 5 and the
    row sits in the smallest LDS hash class whatever the length of its multiplier list: one slot (column C) takes N terms of
    -s * halfp.  N = 60000 is inside the i32 capacity of p = 65521 (65043 terms), N = 70000 beyond it; p = 32749 holds 129 133
    terms, p = 65537 accumulates in i64, and with m > 2N + 10 the bound (N + 5) is not capped and the row goes to the
    global-memory class (i64).  Reference: the closed form of chain_expected; the CPU oracle (canonical arithmetic, iterative
    reach, checked at this depth against the closed form on the CPU: 0.1 s per case) must agree with both."""
    m = N + extra
    assert small == (p < 65536)
    if name.endswith("below_capacity") or name.endswith("capacity_129k"):
        assert N + 1 <= lazy_capacity(p)  # N terms and the row's own entry
    if "70000" in name and p == 65521:
        assert N + 1 > lazy_capacity(p)
    A = chain_matrix(S, p, N, m)
    want = chain_expected(p, N)
    Sc, st, p_out = run_plan(S, A)
    got = Sc.rows()
    lds_ent, big_ent = sum(st["ent_class"][:7]), st["ent_class"][7]
    print(f"{name}: got {got} want {want} entries in LDS classes {lds_ent}, in the global-memory class {big_ent}")
    assert st["npiv"] == N
    assert p_out.tolist() == [N, N + 1]
    assert got == want
    if big is not None:  # the case runs through the class it is meant for
        assert (big_ent > 0) == big and (lds_ent > 0) == (not big), st["ent_class"]
    So, info = O.schur_round(A)
    assert So.rows() == want
    assert info["npiv"] == N
    assert st["applications"] == info["applications"] == 2 * N
    assert st["nnz_reduced"] == info["nnz_reduced"]
    assert st["nnz_out"] == info["nnz_out"] == 10 and st["rows_out"] == info["rows_out"] == 2


def test_echelonize_equal_sign_chain(S):
    """The same matrix (p = 65521, N = 70000, m = N + 5) through echelonize: the round driver sets the scatter up on its own.
    Round 1 elects rows 0..N-1 and leaves the two rows of chain_expected; they lead on column N, one becomes the pivot of column
    N (with v = balanced(-N * h) on C, whichever of the two it is: the other one is its negative on N and C), their sum
    {N+2: 2, N+3: 2, N+4: 2} the last pivot: rank N + 2, columns C, N+3, N+4 free.  U restricted to columns N and C is known
    row by row."""
    p, N = 65521, 70000
    h, Cc = p // 2, N + 1
    A = chain_matrix(S, p, N, N + 5)
    fact = S.echelonize(A, enable_dense=False, **LM)
    v = balanced(-N * h, p)
    print(f"rank {fact.r}, want {N + 2}; rounds {[(r['npiv'], r['rows_out']) for r in S.last_rounds()]}")
    assert fact.r == N + 2
    qinv = np.asarray(fact.qinv)
    assert np.flatnonzero(qinv < 0).tolist() == [Cc, N + 3, N + 4]
    U = fact.U
    nz = int(U.p[U.n])
    Up, Uj, Ux = np.asarray(U.p), np.asarray(U.j[:nz]), np.asarray(U.x[:nz])
    row_of = np.repeat(np.arange(U.n), np.diff(Up))
    sel = np.flatnonzero((Uj == N) | (Uj == Cc))
    got = sorted(zip(row_of[sel].tolist(), Uj[sel].tolist(), Ux[sel].tolist()))
    want = [(int(qinv[i]), Cc, h) for i in range(N)] + [(int(qinv[N - 1]), N, -1), (int(qinv[N]), N, 1), (int(qinv[N]), Cc, v)]
    bad = sorted(set(got) ^ set(want))
    print(f"U on columns N, C: {len(got)} entries, {len(bad)} differ from the closed form: {bad[:8]}")
    assert got == sorted(want)


# ---- (d): the reductions over their stated domains, on the device -----------------------------------------------------------------

SUM_PRIMES = [3, 7, 127, 251, 257, 32749, 65521, 65537, 0xFFFFFFFB]


@pytest.mark.parametrize("p", SUM_PRIMES)
def test_device_lazy_sum_reduction(S, p):
    """spasm_amd_zp_sum_probe: `count` copies of ZpAcc::mul_lazy(a, b) summed in the kernels' accumulator type (i32 for p < 2^16,
    i64 above), then acc_reduce_short -- the reduction every hash class, k_combine and the W build end with.  Operands at the
    edges of the balanced range; counts: 1, 64, the largest LDS table (10240), the documented 60000 and the capacity itself,
    the largest count with count * (halfp + 256) < 2^31 (at most 2^20, what acc_reduce_short is specified for; 0 for
    p = 0xFFFFFFFB, whose empty sum must come out as 0).  p = 65537 and 0xFFFFFFFB accumulate in i64.
    Expected: balanced(count * a * b mod p) in Python integers."""
    lib = S._abi.lib()
    half, mhalf = p // 2, p // 2 - p + 1
    ops = sorted({v for v in (1, -1, half, -half, half - 1, mhalf, half // 2, -(half // 2)) if mhalf <= v <= half})
    cap = min(lazy_capacity(p), 1 << 20)
    counts = sorted({1, 64, 10240, 60000, cap})
    assert p >= 65536 or cap >= 60000  # every prime below 2^16 holds 60000 terms: all counts are inside the domain
    a, b, cnt = [], [], []
    for x in ops:
        for y in ops:
            for c in counts:
                a.append(x); b.append(y); cnt.append(c)
    n = len(a)
    A = np.asarray(a, dtype=np.int32); B = np.asarray(b, dtype=np.int32); Cn = np.asarray(cnt, dtype=np.int32)
    out = np.full(n, 0x55555555, dtype=np.int32)
    P = C.POINTER(C.c_int32)
    rc = lib.spasm_amd_zp_sum_probe(p, n, A.ctypes.data_as(P), B.ctypes.data_as(P), Cn.ctypes.data_as(P), out.ctypes.data_as(P))
    assert rc == 0, S._abi.last_error()
    want = [balanced(c * x * y, p) for x, y, c in zip(a, b, cnt)]
    bad = [(x, y, c, int(g), w) for x, y, c, g, w in zip(a, b, cnt, out, want) if int(g) != w]
    print(f"p = {p}: {n} sums, counts {counts}, {len(bad)} wrong: {bad[:8]}")
    assert not bad
