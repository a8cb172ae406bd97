"""The dense finishes at their digit, accumulator and prime-class boundaries: designed inputs (dense_bounds_cases.py, proved on the
host by test_dense_bounds_host.py) whose block updates sum K products of equal sign and largest magnitude, against their closed
form -- rank, pivot columns, pivot rows and every entry of U, exactly.  Random residues, which is all the other tests feed the
finishes, keep the partial sums near sqrt(K) p and every prime class to four primes.

Every case asserts that the whole matrix went to the dense finish with no sparse round before it (no round record, the
"finishing; density" line, rows and columns of S.dense_stats()) and WHICH finish took it (S.dense_stats()["kind"], its block width)."""
import ctypes as C

import numpy as np
import pytest
from conftest import LM

import dense_bounds_cases as B

pytestmark = pytest.mark.gpu

P_BAND_EDGE = B.next_prime(65279)
P_ABOVE_2_24 = B.next_prime(1 << 24)
TWO_DIGITS = [65521, 65519, 257, 32749, P_BAND_EDGE]
ENV_KEYS = ("SPASM_AMD_TALL", "SPASM_AMD_TALL_SLAB", "SPASM_AMD_TALL_BATCH", "SPASM_AMD_DENSE_KB", "SPASM_AMD_PANEL_GLOBAL", "SPASM_AMD_GEMM_GLDS",
            "SPASM_AMD_DENSE_F64")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(S):
    assert S._abi.lib().spasm_amd_device_count() > 0, "no HIP device visible: GPU tests need the MI355X"


def kind_of(p, forced_f64=False):
    """which finish a prime gets (engine.hip: dense_elem_bytes, dense_eliminate_i8, dense_eliminate)"""
    if p < (1 << 16) and not forced_f64:
        return "i8_one_digit" if p <= 255 else "i8_two_digits"
    return "f64_panels" if p <= (1 << 24) else "rank1_updates"


def echelonize_dense(S, monkeypatch, D, p, env):
    """echelonize the dense matrix D under `env`; returns (A, fact, stats) after asserting that all of it went to a dense finish
    at round 0."""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SPASM_AMD_TALL", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    A = S.CSR(D.T.copy(), prime=p)           # CSR(dense) stores the transpose: the rows of A are the rows of D
    assert A.shape == D.shape and S.nnz(A) == np.count_nonzero(D)
    lines = []
    cb = S.api._LOGFUNC(lambda s: lines.append(s.decode()) or 0)
    slot = C.c_void_p.in_dll(S._abi.lib(), "logcallback")
    prev = slot.value
    slot.value = C.cast(cb, C.c_void_p).value
    try:
        fact = S.echelonize(A, verbose=True, **LM)
    finally:
        slot.value = prev
    st = S.dense_stats()
    assert S.last_rounds() == [], "a sparse round ran before the dense finish"
    assert sum("[echelonize] finishing; density" in x for x in lines) == 1, lines
    assert not any("GPLU" in x or "not enough pivots" in x for x in lines), lines
    return A, fact, st


def check_closed_form(S, A, fact, cols, rows, U, seed=9):
    """rank, pivot columns, the input row of every pivot and every entry of U against the closed form; then the library's own check"""
    q = np.asarray(fact.qinv)
    assert fact.r == len(cols)
    assert np.flatnonzero(q >= 0).tolist() == cols
    k = q[cols]
    assert sorted(k.tolist()) == list(range(fact.r))
    assert np.asarray(fact.p)[k].tolist() == rows
    Ud = fact.U.todense()
    assert Ud.shape == U.shape
    bad = np.argwhere(Ud[k] != U)
    assert bad.size == 0, (len(bad), bad[:5].tolist(), Ud[k][tuple(bad[0])], U[tuple(bad[0])])
    assert S.factorization_verify(A, fact, seed)


def run_designed(S, monkeypatch, p, K, r, c, pattern, env, kind, block, upper=True, extra=0):
    """one designed matrix (plus `extra` rows that repeat its first rows: they vanish) through one finish"""
    D, _, _ = B.designed(p, K, r, c, pattern, upper=upper)
    if extra:
        D = np.vstack([D, D[:extra]])
    A, fact, st = echelonize_dense(S, monkeypatch, D, p, env)
    assert (st["rows"], st["cols"]) == D.shape, st
    assert (st["kind"], st["block"], st["eliminations"], st["tall_finishes"]) == (kind, block, 1, 0), st
    cols, rows, U = B.expected(p, K, r, c, pattern, upper=upper)
    check_closed_form(S, A, fact, cols, rows, U)
    return fact


# ---- 1. one digit: |acc| <= K 127^2 < 2^25 for K <= 2048, zp_small_lazy and one correction ------------------------------------

@pytest.mark.parametrize("pattern", B.PATTERNS)
@pytest.mark.parametrize("p", [251, 127, 3, 7])
def test_one_digit_block_of_2048(S, monkeypatch, p, pattern):
    """K at its stated maximum (SPASM_AMD_DENSE_KB=2048): the update right of the block sums 2048 products (+-h)(+-h) per entry,
    32 000 000 for p = 251 against the 2^25 = 33 554 432 the comment of k_gemm_i8 states; p = 3 and 7: h = 1 and 3."""
    run_designed(S, monkeypatch, p, 2048, 192, 128, pattern, dict(SPASM_AMD_DENSE_KB="2048"), "i8_one_digit", 2048)


@pytest.mark.parametrize("pattern", B.PATTERNS)
@pytest.mark.parametrize("p", [251, 127])
def test_one_digit_default_block(S, monkeypatch, p, pattern):
    """the default block, no override: K = 1024"""
    run_designed(S, monkeypatch, p, 1024, 192, 128, pattern, {}, "i8_one_digit", 1024)


@pytest.mark.parametrize("pattern", B.PATTERNS)
def test_one_digit_single_panel(S, monkeypatch, pattern):
    """K = 64: one panel, the update comes from k_trsm_i8 and one GEMM of K = 64 only"""
    run_designed(S, monkeypatch, 251, 64, 192, 128, pattern, dict(SPASM_AMD_DENSE_KB="64"), "i8_one_digit", 64)


@pytest.mark.parametrize("pattern", B.PATTERNS)
@pytest.mark.parametrize("p", [251, 65521], ids=["one_digit", "two_digits"])
def test_tile_edges_carry_worst_case_values(S, monkeypatch, p, pattern):
    """1197 x 1163: rows and columns that are no multiple of 128, 64 or 16, so that the last tiles of k_gemm_i8 hold rows without
    a target (gi < 0) and columns beyond jb (col0 + e >= jb) next to entries at the bound"""
    run_designed(S, monkeypatch, p, 1024, 173, 139, pattern, {}, kind_of(p), 1024)


@pytest.mark.parametrize("pattern", B.PATTERNS)
def test_one_digit_block_of_2048_panel_rows_in_global_memory(S, monkeypatch, pattern):
    """the same input with the panel kernel working in place (SPASM_AMD_PANEL_GLOBAL=1)"""
    run_designed(S, monkeypatch, 251, 2048, 192, 128, pattern, dict(SPASM_AMD_DENSE_KB="2048", SPASM_AMD_PANEL_GLOBAL="1"), "i8_one_digit", 2048)


@pytest.mark.parametrize("pattern", B.PATTERNS)
def test_one_digit_block_of_2048_lds_dma_gemm(S, monkeypatch, pattern):
    """SPASM_AMD_GEMM_GLDS=1: k_gemm_i8_glds takes the updates with K >= 256 of more than 4096 rows on at least 1024 columns --
    here the one right of the block: K = 2048, 1088 columns (no multiple of its 256-column tile), 4102 rows of which the last 1990
    repeat the first ones and vanish.  The same answer as without the switch, entry for entry."""
    K, r, c, extra = 2048, 64, 1088, 1990
    env = dict(SPASM_AMD_DENSE_KB="2048", SPASM_AMD_GEMM_GLDS="1")
    got = run_designed(S, monkeypatch, 251, K, r, c, pattern, env, "i8_one_digit", 2048, extra=extra)
    assert K + r + extra >= 4096 and c >= 1024
    del env["SPASM_AMD_GEMM_GLDS"]
    ref = run_designed(S, monkeypatch, 251, K, r, c, pattern, env, "i8_one_digit", 2048, extra=extra)
    assert np.array_equal(got.U.p, ref.U.p) and np.array_equal(got.U.todense(), ref.U.todense())


# ---- 2. two digits: the band of zp_digits, three accumulators, the 64-bit recombination ----------------------------------------

@pytest.mark.parametrize("pattern", B.PATTERNS)
@pytest.mark.parametrize("K", [2048, 1024])
@pytest.mark.parametrize("p", TWO_DIGITS, ids=["65521", "65519", "257", "32749", "first_above_65279"])
def test_two_digits_equal_signs(S, monkeypatch, p, K, pattern):
    """p = 65521, 65519: h lies in the band zp_digits moves to [-32896, -32761] (h -> 7 - 128 * 256), so the d1 d1 accumulator
    takes K * 128^2 = 2^25 and the recombination 2^41; 257: the first prime with two digits and shorts; 32749: no band; the
    smallest prime above 65279: the first with a band (computed, and proved prime, here)."""
    assert B.is_prime(P_BAND_EDGE) and P_BAND_EDGE > 65279 and not any(B.is_prime(x) for x in range(65280, P_BAND_EDGE))
    env = dict(SPASM_AMD_DENSE_KB="2048") if K == 2048 else {}
    run_designed(S, monkeypatch, p, K, 192, 128, pattern, env, "i8_two_digits", K)


@pytest.mark.parametrize("K", [2048, 1024])
@pytest.mark.parametrize("p", [65521, 65519, P_BAND_EDGE], ids=["65521", "65519", "first_above_65279"])
def test_two_digits_band_edges(S, monkeypatch, p, K):
    """multipliers and entries of Ut run through 32639, 32640, h, -h and -32768 + p (both edges of the band, the balanced extremes,
    the most negative representative): all 25 pairs, all four sign combinations of d0 d1 + d1 d0"""
    env = dict(SPASM_AMD_DENSE_KB="2048") if K == 2048 else {}
    run_designed(S, monkeypatch, p, K, 192, 128, "band", env, "i8_two_digits", K)


# ---- 3. the f64 panels (2^16 <= p <= 2^24: 64 (p/2)^2 < 2^53 for balanced operands) and the rank-1 updates above ---------------

@pytest.mark.parametrize("pattern", B.PATTERNS)
@pytest.mark.parametrize("p", [65537, 16777213, P_ABOVE_2_24, 2147483647, 0xFFFFFFFB], ids=["65537", "last_below_2_24", "first_above_2_24", "2_31_m1", "0xFFFFFFFB"])
def test_f64_panels_and_rank1_updates(S, monkeypatch, p, pattern):
    """three panels of DPB = 64 pivots (K = 192) and the remainder: every panel's update sums 64 products (+-h)(+-h) in f64 --
    64 h^2 = 2^52 (1 - 7e-7) at 16777213, the stated limit.  Which finish ran is asserted on either side of 2^24."""
    assert B.is_prime(P_ABOVE_2_24) and not any(B.is_prime(x) for x in range((1 << 24) + 1, P_ABOVE_2_24)) and B.prev_prime(1 << 24) == 16777213
    kind = kind_of(p)
    assert kind == ("f64_panels" if p in (65537, 16777213) else "rank1_updates")
    run_designed(S, monkeypatch, p, 192, 192, 128, pattern, {}, kind, 64 if kind == "f64_panels" else 1)


@pytest.mark.parametrize("p", [65537, 16777213], ids=["65537", "last_below_2_24"])
def test_f64_panels_need_balanced_operands(S, monkeypatch, p):
    """multipliers and entries of Ut all -2: nothing as balanced residues, but p - 2 each as canonical ones -- 64 odd products
    (p - 2)^2 pass 2^53 at 16777213, where "64 (p/2)^2 < 2^53" holds for balanced operands only"""
    run_designed(S, monkeypatch, p, 192, 192, 128, "minus2", {}, "f64_panels", 64)


@pytest.mark.parametrize("pattern", B.PATTERNS)
@pytest.mark.parametrize("p", [251, 65521])
def test_f64_panels_forced_for_small_primes(S, monkeypatch, p, pattern):
    """SPASM_AMD_DENSE_F64=1: the f64 panels for primes the int8 finish would take"""
    run_designed(S, monkeypatch, p, 192, 192, 128, pattern, dict(SPASM_AMD_DENSE_F64="1"), "f64_panels", 64)


# ---- 4. tall and skinny: the rows beyond the slab against its reduced form, K = the slab's pivots ----------------------------

@pytest.mark.parametrize("pattern", B.PATTERNS)
@pytest.mark.parametrize("p", [127, 251, 257, 65521])
def test_tall_and_skinny_equal_signs(S, monkeypatch, p, pattern):
    """SPASM_AMD_TALL=1 with a slab of K = 1024 rows: the slab's rows are the K pivots (the left K x K part of Ut is the identity,
    so the reduced form Z of the slab is Ut's right part, u[s] everywhere), every row after them is l[s] times all K slab rows plus
    E, and its reduction t = d_N - d_P Z is one K-term product of equal signs per entry.  K = 1024 is the edge: TallWork reduces
    at most KB = 1024 pivots per GEMM (dense_tall.hpp), and k_gemm_i8 allows 2048.  Two batches of rows.  The result is the closed
    form, and what the plain finish (SPASM_AMD_TALL=0) returns."""
    K, r, c = B.TALL_KB, 192, 128
    D, _, _ = B.designed(p, K, r, c, pattern, upper=False)
    cols, rows, U = B.expected(p, K, r, c, pattern, upper=False)
    A, fact, st = echelonize_dense(S, monkeypatch, D, p, dict(SPASM_AMD_TALL="1", SPASM_AMD_TALL_SLAB=str(K), SPASM_AMD_TALL_BATCH="128"))
    assert st["tall_finishes"] == 1 and st["eliminations"] == 2 and st["kind"] == kind_of(p), st   # the slab, then the residuals
    assert (st["rows"], st["cols"]) == (r, c), st                                                    # (the last one: r x c, E)
    check_closed_form(S, A, fact, cols, rows, U)
    A2, plain, st2 = echelonize_dense(S, monkeypatch, D, p, {})
    assert (st2["tall_finishes"], st2["eliminations"], st2["rows"], st2["cols"]) == (0, 1, K + r, K + c), st2
    check_closed_form(S, A2, plain, cols, rows, U)
    assert np.asarray(fact.qinv).tolist() == np.asarray(plain.qinv).tolist() and np.array_equal(fact.U.todense(), plain.U.todense())


# ---- 5. boundary primes on ordinary data ----------------------------------------------------------------------------------------

BOUNDARY_PRIMES = [3, 7, 127, 251, 257, 32749, P_BAND_EDGE, 65519, 65521, 65537, 16777213, P_ABOVE_2_24, 2147483647, 0xFFFFFFFB]


@pytest.mark.parametrize("p", BOUNDARY_PRIMES)
def test_boundary_primes_on_a_rank_deficient_matrix(S, monkeypatch, p):
    """300 x 260 of rank <= 100 (a product of random factors, a zero column, a dependent column among the first) through every
    prime at a class boundary: rank, pivot columns and the unique reduced echelon form (S.rref) against a Python-integer
    elimination under the same pivot rule -- a wrong storage type or a wrong class at a boundary shows here whatever the designed
    inputs do."""
    D = B.low_rank(p, 300, 260, 100, seed=0xB0)
    prow, pcol, U, _ = B.eliminate(D, p)
    want = B.reduced_form(U, pcol, p)
    A, fact, st = echelonize_dense(S, monkeypatch, D, p, {})
    live = int(np.count_nonzero(np.any(D != 0, axis=0)))
    assert (st["kind"], st["rows"], st["cols"], st["eliminations"]) == (kind_of(p), 300, live, 1), st
    q = np.asarray(fact.qinv)
    assert fact.r == len(pcol) < live and np.flatnonzero(q >= 0).tolist() == pcol
    assert np.asarray(fact.p)[q[pcol]].tolist() == prow
    assert np.array_equal(fact.U.todense()[q[pcol]], U)
    R, rq = S.rref(fact)
    assert R.n == fact.r and np.flatnonzero(rq >= 0).tolist() == pcol
    assert np.array_equal(R.todense()[rq[pcol]], want)
    assert S.factorization_verify(A, fact, 5)
