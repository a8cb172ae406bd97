"""Pins the four Wiedemann families (minpoly, wiedemann_solve, wiedemann_rank, wiedemann_det) on what the commit before their
drivers were folded into one sequence-and-recurrence pipeline computed: tests/golden/wiedemann_family_parent.json holds, for the
fixed cases below, the results and every stat that is not a time (all keys but *_device_us), recorded with that commit's build.
This tree must reproduce every value, and the three entries of a family (CSR, SpMV operator, DeviceCSR) must agree with each
other on both.  Solutions are recorded as the SHA-256 of their int32 bytes.

Cases, for the primes 251 (the SMALL path) and 4294967291 (the wide path):
  * 70 x 70 random matrices, one regular and one singular, K in {1, 3, 8, 64}, tries = 2: minpoly, wiedemann_solve with both trans
    values, wiedemann_det; wiedemann_rank on a 70 x 50 and a 50 x 70 matrix of rank 30;
  * n = 16400, A = I with three rows replaced: a full one (longer than SPMV_SEG = 16384: segments and the combine), one of 40
    entries (a medium row) and one of 5.  A - I has rank <= 3, so the minimal polynomial has degree <= 4 and maxdeg = 8 holds:
    minpoly and wiedemann_solve run 18 terms; wiedemann_rank with maxdeg = 8 runs on the 3 x 16400 matrix of those rows and on
    its transpose.
The determinant is not run at n = 16400: its sequence has 2 n terms, and its long rows go through the same call of the shared
sequence driver as the cases above (the one-set-per-step mode differs from the plain one in the epilogue only)."""
import hashlib
import json
import os

import numpy as np
import pytest

import sparse_worst_cases as SW
from wiedemann_ref import Mat

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wiedemann_family_parent.json")
PRIMES = (251, 4294967291)
KS = (1, 3, 8, 64)
SPMV_SEG = 16384
BIG_N, BIG_K, BIG_MAXDEG = 16400, 3, 8


def mat_rank(D, p):
    """the rank of the dense D mod p (float-free: int64 rows, p < 2^32 through Python integers)"""
    A = [[int(x) % p for x in row] for row in D.tolist()]
    r = 0
    for c in range(len(A[0])):
        piv = next((i for i in range(r, len(A)) if A[i][c]), None)
        if piv is None:
            continue
        A[piv], A[r] = A[r], A[piv]
        inv = pow(A[r][c], -1, p)
        for i in range(r + 1, len(A)):
            if A[i][c]:
                f = A[i][c] * inv % p
                A[i] = [(x - f * y) % p for x, y in zip(A[i], A[r])]
        r += 1
    return r


def small_inputs(p):
    """name -> Mat: `regular` and `singular` 70 x 70 (the last row of the singular one is three times its first), `wide` 50 x 70
    and `tall` 70 x 50 of rank 30; and the right-hand sides K -> B (70 x K, any int32)"""
    rng = np.random.default_rng(20261020 + p % 1000)
    while True:
        D = np.where(rng.random((70, 70)) < 0.15, rng.integers(1, p, size=(70, 70)), 0).astype(np.int64)
        if mat_rank(D, p) == 70:
            break
    Sg = D.copy()
    Sg[69] = 3 * D[0] % p
    out = {"regular": Mat.from_dense(D), "singular": Mat.from_dense(Sg)}
    for name, (n, m) in (("tall", (70, 50)), ("wide", (50, 70))):
        while True:
            L, Rt = rng.integers(0, p, size=(n, 30)).astype(object), rng.integers(0, p, size=(30, m)).astype(object)
            P = np.array(((L @ Rt) % p).tolist(), dtype=np.int64)
            if mat_rank(P, p) == 30:
                break
        out[name] = Mat.from_dense(P)
    return out, {K: SW.rand_int32(rng, (70, K)) for K in KS}


def big_inputs(p):
    """(A, rows, rows^T, B): A = I with rows 0, 1, 2 replaced by a full row, one of 40 entries and one of 5 (each keeps a non-zero
    diagonal entry); rows is the 3 x n matrix of the three"""
    rng = np.random.default_rng(777 + p % 1000)
    n = BIG_N
    assert n > SPMV_SEG
    three = [[(j, int(rng.integers(1, p))) for j in range(n)]]
    for i, cnt in ((1, 40), (2, 5)):
        cols = sorted({i} | {int(c) for c in rng.choice(n, size=cnt - 1, replace=False) if c != i})
        three.append([(c, int(rng.integers(1, p))) for c in cols])
    assert len(three[0]) > SPMV_SEG and 32 < len(three[1]) <= 40 and 1 < len(three[2]) <= 5
    A = Mat.from_rows(three + [[(i, 1)] for i in range(3, n)], n)
    rows = Mat.from_rows(three, n)
    return A, rows, rows.transpose(), SW.rand_int32(rng, (n, BIG_K))


def nontiming(st):
    return {k: v for k, v in st.items() if not k.endswith("_device_us")}


def three_entries(S, A, call, stats):
    """[{result, stats}] of call(handle) through the CSR, the SpMV operator and the DeviceCSR of A"""
    out = []
    with S.SpMV(A) as op, S.DeviceCSR(A) as D:
        for h in (A, op, D):
            res = call(h)
            out.append(json.loads(json.dumps({"result": res, "stats": nontiming(stats())})))
    return out


def solve_record(S, h, B, **kw):
    X, status = S.wiedemann_solve(h, B, **kw)
    assert X.dtype == np.int32 and X.shape == B.shape
    return {"X_sha256": hashlib.sha256(np.ascontiguousarray(X).tobytes()).hexdigest(), "status": status.tolist()}


def small_cases(S, p):
    """key -> the three records of the 70 x 70 group"""
    mats, rhs = small_inputs(p)
    csr = {name: M.csr(S, p) for name, M in mats.items()}
    out = {}
    for K in KS:
        B = rhs[K]
        out[f"minpoly_K{K}"] = three_entries(S, csr["regular"], lambda h: S.minpoly(h, K=K, seed=5).tolist(), S.minpoly_stats)
        for name in ("regular", "singular"):
            for trans in (False, True):
                out[f"solve_{name}_trans{int(trans)}_K{K}"] = three_entries(
                    S, csr[name], lambda h: solve_record(S, h, B, trans=trans, seed=7, tries=2), S.wiedemann_stats)
            out[f"det_{name}_K{K}"] = three_entries(S, csr[name], lambda h: list(S.wiedemann_det(h, K=K, seed=11, tries=2)), S.precond_stats)
        for name in ("tall", "wide"):
            out[f"rank_{name}_K{K}"] = three_entries(S, csr[name], lambda h: list(S.wiedemann_rank(h, K=K, seed=3, tries=2)), S.precond_stats)
    return out


def big_cases(S, p):
    """key -> the three records of the n = 16400 group"""
    A, rows, rows_t, B = big_inputs(p)
    K, md = BIG_K, BIG_MAXDEG
    a = A.csr(S, p)
    out = {"minpoly": three_entries(S, a, lambda h: S.minpoly(h, K=K, seed=5, maxdeg=md).tolist(), S.minpoly_stats)}
    for trans in (False, True):
        out[f"solve_trans{int(trans)}"] = three_entries(
            S, a, lambda h: solve_record(S, h, B, trans=trans, seed=7, tries=2, maxdeg=md), S.wiedemann_stats)
    for name, M in (("rows", rows), ("rows_t", rows_t)):
        out[f"rank_{name}"] = three_entries(
            S, M.csr(S, p), lambda h: list(S.wiedemann_rank(h, K=K, seed=3, tries=2, maxdeg=md)), S.precond_stats)
    return out


GROUPS = {"small": small_cases, "big": big_cases}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("p", PRIMES)
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_results_and_stats_equal_the_recorded_parent(S, golden, group, p):
    got = GROUPS[group](S, p)
    want = golden[f"{group}_p{p}"]
    assert sorted(got) == sorted(want)
    for key, recs in got.items():
        print(key, recs[0])
        assert recs[1] == recs[0] and recs[2] == recs[0], (key, "the three entries disagree", recs)
        assert recs[0] == want[key], (key, recs[0], want[key])
    if group == "big":   # every product went through the short rows, the segments of the long one and the combine at least
        assert want["minpoly"]["stats"]["steps"] == 2 * BIG_MAXDEG + 1
        assert want["minpoly"]["stats"]["launches"] >= 3 * want["minpoly"]["stats"]["steps"]
        assert want["solve_trans0"]["stats"]["launches"] >= 3 * want["solve_trans0"]["stats"]["products"]
