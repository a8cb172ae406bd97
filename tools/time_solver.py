"""Times the resident solver (csrc/solver.hpp) against S.solve_batch called again for every set of right-hand sides, which is all
the engine could do before: (i) N = 100, 1000, 10000 systems of 50 x 60 (synth_csr kind 0, density 0.1) with K = 1, 4, 64
right-hand sides each (every second one y * A, the others random) at p = 65521 and p = 127, (ii) a block matrix of 5000 connected
components of mixed sizes with a 1000-row Rhs, DeviceBlocks.solver().solve against DeviceBlocks.solve.  Per case: wall
microseconds per system of solver.solve and of solve_batch (both the median of --reps calls after --warmup), their ratio, the wall
time of the create, the number of applies after which create + applies is cheaper than as many solve_batch calls, and the device
microseconds both sides report.  The results of both sides are compared byte for byte.  One JSON line per case, appended to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spasm_jl_amd as S  # noqa: E402
from time_batch import block_matrix  # noqa: E402


def timed(fn, reps, warmup):
    us, out = [], None
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        out = fn()
        if r >= warmup:
            us.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(us)), out


def raw(X):
    nz = int(X.p[X.n])
    return X.p.tobytes() + X.j[:nz].tobytes() + X.x[:nz].tobytes()


def rhs_for(A, K, p, rng):
    """K right-hand sides: the even ones combinations of three rows of A, the odd ones random and sparse"""
    rows = A.rows()
    out = []
    for k in range(K):
        acc = {}
        if k % 2 == 0:
            for i in rng.integers(0, A.n, size=3):
                f = int(rng.integers(1, p))
                for c, v in rows[int(i)]:
                    acc[c] = (acc.get(c, 0) + f * v) % p
        else:
            for c in rng.integers(0, A.m, size=6):
                acc[int(c)] = int(rng.integers(1, p))
        out.append(sorted((c, v - p if 2 * v > p else v) for c, v in acc.items() if v))
    return S.CSR.from_rows(out, A.m, prime=p)


def report(out_path, name, systems, apply_us, batch_us, create_us, info, st_apply, st_batch, extra=None):
    gain = batch_us - apply_us
    line = {
        "case": name, "systems": systems, "apply_us_per_system": round(apply_us / systems, 3), "solve_batch_us_per_system": round(batch_us / systems, 3),
        "ratio_solve_batch_over_apply": round(batch_us / max(apply_us, 1e-9), 2), "create_us": round(create_us, 1),
        "break_even_applies": (int(np.ceil(create_us / gain)) if gain > 0 else None), "apply_device_us": st_apply["device_us"],
        "solve_batch_device_us": st_batch["device_us"], "apply_jobs": st_apply["jobs"], "solve_batch_jobs": st_batch["jobs"], **{"info_" + k: v for k, v in info.items()},
    }
    line.update(extra or {})
    text = json.dumps(line)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="100,1000,10000")
    ap.add_argument("--rhs", default="1,4,64")
    ap.add_argument("--primes", default="65521,127")
    ap.add_argument("--components", type=int, default=5000, help="0: skip the block case")
    ap.add_argument("--rhs-rows", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "solver_timing.jsonl"))
    a = ap.parse_args()
    for p in [int(v) for v in a.primes.split(",")]:
        for N in [int(v) for v in a.sizes.split(",")]:
            mats = [S.synth_csr(0, 50, 60, density=0.1, prime=p, seed=0x501E0000 + k) for k in range(N)]
            t0 = time.perf_counter()
            sv = S.BatchSolver(mats)
            create_us = (time.perf_counter() - t0) * 1e6
            for K in [int(v) for v in a.rhs.split(",")]:
                rng = np.random.default_rng(0x501E + K)
                rhs = [rhs_for(A, K, p, rng) for A in mats]
                apply_us, (X, ok) = timed(lambda: sv.solve(rhs), a.reps, a.warmup)
                st_apply = S.solver_stats()
                batch_us, (Xw, okw) = timed(lambda: S.solve_batch(mats, rhs), a.reps, a.warmup)
                st_batch = S.solve_stats()
                assert all(raw(x) == raw(y) and np.array_equal(o, q) for x, y, o, q in zip(X, Xw, ok, okw)), "solver and solve_batch disagree"
                report(a.out, f"50x60_p{p}_N{N}_K{K}", N, apply_us, batch_us, create_us, sv.info(), st_apply, st_batch, {"unsolved": st_apply["unsolved"]})
                del X, Xw, rhs
            sv.close()
    if a.components > 0:
        p = 42013
        A = block_matrix(a.components, 0xB10C, p)
        rng = np.random.default_rng(0xB10C)
        rows = A.rows()
        rr = []
        for k in range(a.rhs_rows):
            acc = {}
            for i in rng.integers(0, A.n, size=4):
                f = int(rng.integers(1, p))
                for c, v in rows[int(i)]:
                    acc[c] = (acc.get(c, 0) + f * v) % p
            if k % 4 == 3:
                acc[int(rng.integers(0, A.m))] = 1
            rr.append(sorted((c, v - p if 2 * v > p else v) for c, v in acc.items() if v))
        Rhs = S.CSR.from_rows(rr, A.m, prime=p)
        with S.DeviceBlocks(A) as db:
            t0 = time.perf_counter()
            sv = db.solver()
            create_us = (time.perf_counter() - t0) * 1e6
            apply_us, (X, ok) = timed(lambda: sv.solve(Rhs), a.reps, a.warmup)
            st_apply = S.solver_stats()
            batch_us, (Xw, okw) = timed(lambda: db.solve(Rhs), a.reps, a.warmup)
            st_batch = S.solve_stats()
            assert raw(X) == raw(Xw) and np.array_equal(ok, okw), "solver and blocks solve disagree"
            report(a.out, f"block_{len(db)}_components_rhs{a.rhs_rows}", len(db), apply_us, batch_us, create_us, sv.info(), st_apply, st_batch,
                   {"shape": list(A.shape), "nnz": S.nnz(A), "unsolved": st_apply["unsolved"]})
            sv.close()


if __name__ == "__main__":
    main()
