"""Times the batched solve of small systems (csrc/solve_batch.hpp) against the only way to solve them without it, a loop of
S.echelonize(A, L=True) + S.gesv per matrix: (i) N = 100, 1000, 10000 random 50 x 60 matrices (synth_csr kind 0, density 0.1) with
K = 4 right-hand sides each (two of them y * A, two random) at p = 65521 and p = 127; (ii) the block matrix of tools/time_batch.py
(5000 connected components) with a 1000-row right-hand side through S.DeviceBlocks.solve, against the host-Block route
(S.blocks.solve on Block.from_csr: one solve_batch call) and against the per-block loop of echelonize(L=True) + gesv.
Per case: wall us per system of the batch call (median of --reps after --warmup calls) and of the loop (one pass after a warm-up
of 20 systems, over the first --loop-max systems: the loop's cost per system does not depend on N), their ratio, and solve_stats
of the last batch call.  ok of both sides is compared.  One JSON line per case; --out appends them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spasm_jl_amd as S  # noqa: E402
from tools.time_batch import block_matrix, timed_batch  # noqa: E402


def rhs_for(A, K, rng):
    """K rows over A's prime: the even ones y * A for a sparse y, the odd ones random"""
    p, (n, m) = A.prime, A.shape
    D = np.zeros((n, m), dtype=np.int64)
    for i, r in enumerate(A.rows()):
        for c, v in r:
            D[i, c] = v % p
    rows = []
    for k in range(K):
        if k % 2 == 0:
            y = rng.integers(0, p, size=n) * (rng.random(n) < 0.3)
            b = (y @ D) % p
        else:
            b = rng.integers(0, p, size=m) * (rng.random(m) < 0.3)
        rows.append([(int(c), int(b[c])) for c in np.nonzero(b)[0]])
    return S.CSR.from_rows(rows, m, prime=p)


def loop(mats, rhs, loop_max):
    for A, B in list(zip(mats, rhs))[:20]:
        S.gesv(S.echelonize(A, L=True), B)
    part = list(zip(mats, rhs))[:loop_max]
    t0 = time.perf_counter()
    oks = [S.gesv(S.echelonize(A, L=True), B)[1].tolist() for A, B in part]
    return (time.perf_counter() - t0) * 1e6 / max(len(part), 1), oks


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="100,1000,10000")
    ap.add_argument("--primes", default="65521,127")
    ap.add_argument("--rhs", type=int, default=4)
    ap.add_argument("--loop-max", type=int, default=300)
    ap.add_argument("--components", type=int, default=5000, help="0: skip the block case")
    ap.add_argument("--block-rhs", type=int, default=1000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rng = np.random.default_rng(0x501E)
    for p in [int(v) for v in a.primes.split(",")]:
        sizes = [int(v) for v in a.sizes.split(",")]
        mats = [S.synth_csr(0, 50, 60, density=0.1, prime=p, seed=0xBA7C0000 + k) for k in range(max(sizes))]
        rhs = [rhs_for(A, a.rhs, rng) for A in mats]
        loop_us, loop_ok = loop(mats, rhs, a.loop_max)
        for N in sizes:
            ms, (X, ok) = timed_batch(lambda: S.solve_batch(mats[:N], rhs[:N]), a.reps, a.warmup)
            st = S.solve_stats()
            assert [o.tolist() for o in ok[: len(loop_ok)]] == loop_ok[:N], "batch and loop disagree on ok"
            emit({"case": f"50x60_K{a.rhs}_p{p}_N{N}", "systems": N, "batch_us_per_system": round(ms * 1e3 / N, 3), "loop_us_per_system": round(loop_us, 1),
                  "loop_systems": len(loop_ok), "ratio_loop_over_batch": round(loop_us / max(ms * 1e3 / N, 1e-9), 1), "batch_ms": round(ms, 3),
                  "device_us_per_system": round(st["device_us"] / N, 3), **{k: v for k, v in st.items() if k != "systems"}}, a.out)
    if a.components > 0:
        A = block_matrix(a.components, 0xB10C, 42013)
        n, m = A.shape
        import scipy.sparse as sp

        Asp = sp.csr_matrix((A.x[: S.nnz(A)].astype(np.int64) % 42013, A.j[: S.nnz(A)], A.p), shape=(n, m))
        rows = []
        for k in range(a.block_rhs):
            y = sp.csr_matrix((rng.integers(1, 42013, size=40), (np.zeros(40, dtype=np.int64), rng.choice(n, size=40, replace=False))), shape=(1, n))
            b = np.asarray((y @ Asp).todense()).ravel() % 42013
            if k % 2:
                b[rng.choice(m, size=2)] += 1
            rows.append([(int(c), int(b[c] % 42013)) for c in np.nonzero(b % 42013)[0]])
        R = S.CSR.from_rows(rows, m, prime=42013)
        with S.DeviceBlocks(A) as D:
            dev_ms, (X, ok) = timed_batch(lambda: D.solve(R), a.reps, a.warmup)
            st = S.solve_stats()
        Bk = S.Block.from_csr(A)
        host_ms, (Xh, okh) = timed_batch(lambda: S.blocks.solve(Bk, R), 1, 1)
        assert ok.tolist() == okh.tolist() and X.rows() == Xh.rows(), "the device route and the host-Block route disagree"
        # the per-block loop without this change: every block that receives a right-hand side, echelonized with L and solved
        blocks = [Ab for Ab in Bk.blocks if Ab.n > 0 and Ab.m > 0][: a.loop_max]
        t0 = time.perf_counter()
        for Ab in blocks:
            S.gesv(S.echelonize(Ab, L=True), S.CSR.from_rows([[(0, 1)]], Ab.m, prime=42013))
        loop_us = (time.perf_counter() - t0) * 1e6 / max(len(blocks), 1)
        emit({"case": f"block_{len(Bk)}_components_rhs{a.block_rhs}", "shape": [n, m], "nnz": S.nnz(A), "rhs_nnz": S.nnz(R), "device_blocks_ms": round(dev_ms, 3),
              "host_block_ms": round(host_ms, 3), "ratio_host_over_device": round(host_ms / max(dev_ms, 1e-9), 1), "loop_us_per_block": round(loop_us, 1),
              "loop_blocks": len(blocks), "loop_ms_extrapolated": round(loop_us * st["systems"] / 1e3, 1),
              "device_us_per_system": round(st["device_us"] / max(st["systems"], 1), 3), **st}, a.out)


if __name__ == "__main__":
    main()
