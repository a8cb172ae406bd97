"""The constructions of dense_bounds_cases.py, proved with Python integers on the host: what test_gpu_dense_bounds.py takes for
granted.  No GPU, no library: a construction that comes out wrong fails here, not on the device.  The designed matrices are
eliminated at a reduced K (the closed form does not depend on K); the bounds are evaluated at the K the GPU tests run."""
import numpy as np
import pytest

import dense_bounds_cases as B

P_BAND_EDGE = B.next_prime(65279)          # the smallest prime with a band: residues in (32639, h]
P_ABOVE_2_24 = B.next_prime(1 << 24)
ONE_DIGIT = [251, 127, 3, 7]
TWO_DIGITS = [65521, 65519, 257, 32749, P_BAND_EDGE]
F64 = [65537, 16777213]
RANK1 = [P_ABOVE_2_24, 2147483647, 0xFFFFFFFB]
ALL_PRIMES = ONE_DIGIT + TWO_DIGITS + F64 + RANK1


def test_the_primes_are_what_the_cases_say():
    assert all(B.is_prime(p) for p in ALL_PRIMES)
    assert [p for p in range(2, 60) if B.is_prime(p)] == [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59]
    assert not B.is_prime(65521 * 65537) and not B.is_prime(3215031751) and not B.is_prime(0xFFFFFFFF)
    assert B.prev_prime(256) == 251 and B.next_prime(255) == 257            # the one-digit | two-digit switch, F.p <= 255
    assert B.prev_prime(1 << 16) == 65521 and B.next_prime(1 << 16) == 65537
    assert B.prev_prime(1 << 24) == 16777213 and P_ABOVE_2_24 > (1 << 24)    # the f64 panels | rank-1 switch, F.p <= 1 << 24
    assert B.prev_prime(1 << 31) + 1 == 1 << 31 and B.prev_prime(1 << 32) == 0xFFFFFFFB
    assert 65279 < P_BAND_EDGE and not any(B.is_prime(q) for q in range(65280, P_BAND_EDGE))
    # a band exists exactly when h > 32639, i.e. p > 65279
    assert P_BAND_EDGE // 2 > B.BAND_LO and 32749 // 2 <= B.BAND_LO and B.prev_prime(65280) // 2 <= B.BAND_LO
    assert 65521 // 2 > B.BAND_LO and 65519 // 2 > B.BAND_LO


def test_eliminate_is_the_plain_rule():
    """the vectorised eliminator against lists and Python integers, int64 and object entries, a rank-deficient input"""
    for p in (7, 65521, 2147483647, 0xFFFFFFFB):
        M = B.low_rank(p, 23, 90, 9, seed=p % 1000)
        prow, pcol, U, left = B.eliminate(M, p)
        prow2, pcol2, U2 = B.eliminate_plain(M.tolist(), p)
        assert (prow, pcol) == (prow2, pcol2) and U.tolist() == U2
        assert 5 not in pcol and 70 not in pcol and len(pcol) <= 9
        rest = np.delete(left, prow, axis=0)
        assert not rest.any()                                                # rank-deficient: the other rows vanish
        R = B.reduced_form(U, pcol, p)
        for t, c in enumerate(pcol):
            assert R[t, c] == 1 and np.count_nonzero(R[:, c]) == 1


# (the band of zp_digits exists for 65279 < p < 2^16 only)
CLOSED_FORM = ([(p, pat) for p in ALL_PRIMES for pat in B.PATTERNS] + [(p, "band") for p in (65521, 65519, P_BAND_EDGE)]
               + [(p, "minus2") for p in F64])


@pytest.mark.parametrize("upper", [True, False], ids=["upper", "identity"])
@pytest.mark.parametrize("p,pattern", CLOSED_FORM)
def test_designed_matrix_eliminates_to_its_closed_form(p, pattern, upper):
    """pivots, multipliers, rows of U and the remainder E, by the reference elimination of the designed matrix at K = 24"""
    K, r, c = 24, 13, 11
    D, Ut, E = B.designed(p, K, r, c, pattern, seed=3, upper=upper)
    l, u = B.pattern_values(p, K, pattern)
    h = p // 2
    assert D.shape == (K + r, K + c) and np.all(np.abs(D) <= h) and np.all(np.abs(Ut) <= h)
    assert np.all(np.any(D != 0, axis=1)) and np.all(np.any(D != 0, axis=0))    # no row, no column drops out of the finish
    # D is Lm Ut + E in Python integers
    Lm = np.zeros((K + r, K), dtype=object)
    for s in range(K):
        Lm[s, s] = 1
        Lm[s + 1:, s] = int(l[s])
    want = Lm.dot(Ut.astype(object))
    want[K:, K:] += E.astype(object)
    assert ((want - D.astype(object)) % p == 0).all()
    # after K pivots: row s won column s, the rows of U are Ut, the rows >= K hold E and nothing else
    prow, pcol, U, left = B.eliminate(D, p, max_pivots=K)
    assert prow == list(range(K)) and pcol == list(range(K))
    assert np.array_equal(U, Ut)
    assert not left[K:, :K].any() and np.array_equal(left[K:, K:], B.bal(E, p))
    # the multipliers: column s of the rows below s, when its turn comes, is l[s]
    _, _, _, mid = B.eliminate(D, p, max_pivots=K // 2)
    assert np.all(mid[K // 2 + 1:, K // 2] == l[K // 2])
    # all of it: the closed form the GPU tests compare with
    cols, rows, Uexp = B.expected(p, K, r, c, pattern, seed=3, upper=upper)
    prow, pcol, U, _ = B.eliminate(D, p)
    assert (pcol, prow) == (cols, rows) and np.array_equal(U, Uexp)


@pytest.mark.parametrize("p", ONE_DIGIT + TWO_DIGITS)
@pytest.mark.parametrize("pattern", B.PATTERNS)
def test_designed_matrix_stays_dense_at_the_sizes_the_gpu_runs(p, pattern):
    """density well above the 0.05 of sparsity_threshold, no empty row or column: the whole matrix goes to the dense finish"""
    for K, r, c, upper in ((2048, 192, 128, True), (1024, 192, 128, False)):
        D, _, _ = B.designed(p, K, r, c, pattern, upper=upper)
        assert np.count_nonzero(D) > 0.25 * D.size
        assert np.all(np.any(D != 0, axis=1)) and np.all(np.any(D != 0, axis=0))


def test_update_terms_are_equal_and_extreme():
    for p in ALL_PRIMES:
        h = p // 2
        for pattern in ("pp", "pm", "mp", "mm"):
            l, u = B.pattern_values(p, 64, pattern)
            prods = set((l * u).tolist()) if p < (1 << 31) else {int(a) * int(b) for a, b in zip(l, u)}
            assert len(prods) == 1 and abs(prods.pop()) == h * h
        l, u = B.pattern_values(p, 64, "alt")
        assert sum(int(a) * int(b) for a, b in zip(l, u)) == 0 and all(abs(int(a) * int(b)) == h * h for a, b in zip(l, u))


def test_one_digit_bound():
    """dense.hpp, k_gemm_i8: |acc| <= K * 127^2 < 2^25 for K <= 2048; the lazy reduction wants |x / p| < 2^22"""
    assert 2048 * 127 ** 2 < 1 << 25 <= 2081 * 127 ** 2
    for p in ONE_DIGIT:
        acc = B.one_digit_sum(p, B.KB_MAX)
        assert acc <= B.KB_MAX * 127 ** 2 < 1 << 25
        assert (acc + p // 2) // p < 1 << 22
    assert B.one_digit_sum(251, 2048) == 32_000_000                          # 95 % of 2^25: the case that comes nearest
    assert B.one_digit_sum(251, 2048) >= 1 << 24                             # a path that assumes |acc| < 2^24 is wrong here
    assert B.one_digit_sum(127, 2048) < 1 << 24 <= B.one_digit_sum(251, 1074)
    assert [B.one_digit_sum(p, 2048) // p for p in (3, 7)] == [682, 2633]    # h = 1 and 3: the quotient of the lazy step in units of p


def test_two_digit_ranges_and_accumulators():
    """dense.hpp, zp_digits and the three accumulators of k_gemm_i8, at K = 2048"""
    for p in TWO_DIGITS:
        h = p // 2
        edge = sorted({-h, -h + 1, -129, -128, -1, 0, 1, 127, 128, B.BAND_LO - 1, B.BAND_LO, min(B.BAND_LO + 1, h), h - 1, h})
        for v in edge:
            d0, d1 = B.zp_digits(v, p)
            assert -128 <= d0 <= 127 and -128 <= d1 <= 127 and (d0 + 256 * d1 - v) % p == 0
            assert -32896 <= d0 + 256 * d1 <= B.BAND_LO
        # without the band branch a residue above 32639 has no second digit that fits a signed byte
        if h > B.BAND_LO:
            v = B.BAND_LO + 1
            d0 = ((v + 128) & 255) - 128
            assert (v - d0) >> 8 == 128
        if -32768 + p > B.BAND_LO:                                           # p > 65407: -32768 has a residue inside the band
            assert -32768 + p <= h and B.zp_digits(-32768 + p, p) == (0, -128)   # the most negative second digit
        for pattern in B.PATTERNS + (("band",) if h > B.BAND_LO else ()):
            l, u = B.pattern_values(p, B.KB_MAX, pattern)
            a0, a1, a2, total = B.two_digit_sums(p, B.KB_MAX, l, u)
            assert abs(a0) <= B.KB_MAX * 128 ** 2 == 1 << 25 and abs(a1) <= 1 << 26 and abs(a2) <= 1 << 25
            assert (total - sum(int(x) * int(y) for x, y in zip(l, u))) % p == 0
            assert abs(total) < 1 << 62                                      # zp_reduce's domain
            if pattern in ("pp", "pm", "mp", "mm") and p > 257:
                assert abs(total) >= 1 << 31                                 # a 32-bit recombination wraps
    # p = 65521, all signs equal: h = 32760 is sent to -32761 = 7 - 128 * 256; the second-digit accumulator is the large one
    l, u = B.pattern_values(65521, 2048, "pp")
    assert B.two_digit_sums(65521, 2048, l, u) == (2048 * 7 * 7, 2048 * 2 * 7 * -128, 2048 * 128 * 128, 2048 * 32761 ** 2)
    # the band values give every sign pair of (d0, d1) x (d0, d1)
    l, u = B.pattern_values(65521, 25, "band")
    digits = [(B.zp_digits(a, 65521), B.zp_digits(b, 65521)) for a, b in zip(l.tolist(), u.tolist())]
    signs = {(int(np.sign(x0 * y1)), int(np.sign(x1 * y0))) for (x0, x1), (y0, y1) in digits}
    assert {(1, 1), (1, -1), (-1, 1), (-1, -1)} <= signs, signs
    assert len(set(zip(l.tolist(), u.tolist()))) == 25


def test_f64_panel_bound_on_both_sides_of_2_24():
    """kernels.hpp: "64 (p/2)^2 < 2^53 for p <= 2^24" holds for balanced operands only; it is not tight -- balanced operands stay
    exact up to p < 2^24.5, so the prime just above 2^24 would still be summed exactly by the f64 panels"""
    for p in F64:
        assert B.f64_panel_sum(p) < 1 << 53
    assert B.f64_panel_sum(16777213) == 64 * 8388606 ** 2 > 0.999 * (1 << 52)   # the stated limit is 2^52 at 2^24
    assert B.f64_panel_sum(16777213, balanced=False) > 1 << 53                   # canonical operands [0, p) are not exact here
    assert B.f64_panel_sum(65537, balanced=False) < 1 << 53
    assert B.f64_panel_sum(P_ABOVE_2_24) < 1 << 53                               # (see above: the clamp at 2^24 is conservative)
    first_inexact = B.next_prime(int(2 ** 24.5))
    assert B.f64_panel_sum(first_inexact) > 1 << 53 > B.f64_panel_sum(B.prev_prime(int(2 ** 24.5)))
    for p in RANK1[1:]:
        assert B.f64_panel_sum(p) > 1 << 53                                      # these need the rank-1 path
    # the pattern "minus2": nothing as balanced operands, (p - 2)^2 odd and 64 of them beyond 2^53 as canonical ones -- the chain of
    # k_panel_trsm2 is then off by one more at every step past 2^53, never by a multiple of p
    p = 16777213
    assert B.pattern_values(p, 64, "minus2")[0].tolist() == [-2] * 64 == B.pattern_values(p, 64, "minus2")[1].tolist()
    assert B.f64_fma_chain(-2, -2, 63) == (-252, -252) and B.f64_fma_chain(p // 2, p // 2, 63)[0] == -63 * (p // 2) ** 2
    got, exact = B.f64_fma_chain(p - 2, p - 2, 63)
    assert (p - 2) ** 2 % 2 == 1 and abs(exact) > 1 << 53 and 0 < abs(got - exact) < p
    got, exact = B.f64_fma_chain(65537 - 2, 65537 - 2, 63)
    assert got == exact                                                          # p = 65537 is exact either way
